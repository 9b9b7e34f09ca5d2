"""Boundary batches of the URI kernels' owner lookup (uri_owner_corpus), CPU
part: the oracle and the emulation of the device per-line code agree on every
line, none is FALLBACK, and each batch holds the quantity it plants -- blocks,
events or pieces per lane, re-derived from the built lines -- so that the GPU
part (test_uri_owner_gpu.py) stands on the boundary it names."""
import copy
import re

import pytest

import uri_owner_corpus as uoc
import uri_wave_corpus as uwc
from test_uri_wave import check

PLAN_NAMES = ["ones", "long0", "long31", "long63", "first63", "first64", "first65", "first127", "first128",
              "first64-run2", "first64-run40"]


def _ok_lines(c):
    return len(c.lines) - len(c.bad)


def _planted(c, got):
    plan = c.info["plan"]
    assert len(c.lines) == 64 and got == plan, (c.name, got, plan)
    t = c.info["target"]
    if t is not None:
        assert got[t] > 0, c.name
        m = re.search(r"-first(\d+)", c.name)
        if m:  # the lane's first item is the one the batch is named after
            assert sum(got[:t]) == int(m.group(1)), (c.name, t, sum(got[:t]))


def test_plans():
    p66, p70 = uoc.plans(66), uoc.plans(70)
    assert list(p66) == PLAN_NAMES == list(p70)
    assert {n: f for n, (_, f) in uoc.targets().items()} == {
        "first63": 63, "first64": 64, "first65": 65, "first127": 127, "first128": 128, "first64-run2": 64,
        "first64-run40": 64}
    for run in (2, 40):
        plan, t = p66["first64-run%d" % run]
        assert plan[t - run:t] == [0] * run and plan[t - run - 1] > 0 and plan[0] == plan[63] == 0
    for lane in (0, 31, 63):
        assert p66["long%d" % lane][0][lane] == 66  # a round of 64 blocks without a head


def test_block_batches(oracle, emu):
    cases = uoc.block_cases()
    assert [c.name for c in cases] == ["OB-" + n for n in PLAN_NAMES]
    for c in cases:
        assert check(oracle, emu, c) == _ok_lines(c)
        _planted(c, uoc.line_blocks(c))
        assert c.wave_blocks() == [sum(c.info["plan"])]
        assert 16 * c.wave_blocks()[0] + 16 <= uoc.URI_CAP, c.name  # the compact buffer of k_uri_lines
        assert all(r is None for (_, r) in c.uris)  # '-' referers
    c = cases[0]
    assert all(s[0][0] // 16 == (s[0][1] - 1) // 16 for s in c.spans)  # each URI inside one aligned block
    long0 = cases[1]
    assert long0.spans[0][0][1] - long0.spans[0][0][0] >= 1040
    c = uoc.block_overflow_case()
    assert check(oracle, emu, c) == 64
    _planted(c, uoc.line_blocks(c))
    assert 9 * 64 < c.wave_blocks()[0] and 16 * c.wave_blocks()[0] + 16 <= 4 * uoc.URI_CAP


@pytest.mark.parametrize("where", ["req", "ref", "both"])
def test_event_batches(oracle, emu, where):
    for c in uoc.event_cases(where):
        assert check(oracle, emu, c) == _ok_lines(c)
        for stage in (0, 1):
            got = uoc.line_events(c, stage)
            if (where, stage) in (("req", 0), ("ref", 1), ("both", 0), ("both", 1)):
                _planted(c, got)
            else:
                assert sum(got) == 0, c.name  # the other stage has no event at all
        assert 16 * c.wave_blocks()[0] + 16 <= uoc.URI_CAP, c.name


@pytest.mark.parametrize("fmt", ["combined", "mixed"])
def test_piece_batches(oracle, emu, fmt):
    for c in uoc.piece_cases(fmt):
        assert check(oracle, emu, c) == _ok_lines(c)
        _planted(c, uoc.line_pieces(c))
        assert c.wave_pieces() == [sum(c.info["plan"])]
        assert 16 * c.wave_blocks()[0] + 16 <= uoc.URI_CAP, c.name
        if fmt == "combined":  # one named parameter and a referer part: the BAD lines are OK, and have no piece
            named = copy.copy(c)
            named.bad = set()
            assert check(oracle, emu, named, fields=uwc.NAMED_FIELDS) == 64
        if fmt == "mixed":
            assert sum(1 for l in c.lines if l.count(b'"') == 2) >= 5, c.name  # 'common' lines among them
