"""Boundary batches of the URI kernels' owner lookup (uri_owner_corpus), GPU
part: one-wave batches in which a line's first block / event / piece falls on
item 63, 64, 65, 127, 128 of the wave, a lane holds more than a round of
items (a round without a head), item-less lanes (BAD lines, lines without a
request) sit in lanes 0 and 63 and in runs of 2 and 40 directly before the
line that starts on item 64.  Every line against the oracle, bit-exact; no
FALLBACK, arena_ovf 0, uri_repair_lines 0 (decided / decided_with of
test_uri_wave_gpu).  The CPU part, which validates the batches and what they
plant, is test_uri_owner.py."""
import functools

import pytest

import logparser_amd as lpa
import uri_owner_corpus as uoc
import uri_wave_corpus as uwc
from test_uri_wave_gpu import _parser, decided, decided_with

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def _pieces(fmt="combined"):
    return uoc.piece_cases(fmt)


def _all(oracle, cases, fields=None, options=None, overflow=0):
    p = None
    for c in cases:
        p = p or _parser(oracle, c, fields=fields, options=options)
        r = decided_with(oracle, c, p)
        if fields is None:  # (named fields leave the time stamp alone: its BAD lines are OK, as in the oracle)
            assert r.counters["bad"] == len(c.bad), (c.name, r.counters)
        if overflow is not None:
            assert r.diag["uri_overflow_waves"] == overflow, (c.name, r.diag)


# ------------------------------------------------------------------ blocks
def test_owner_blocks_gpu(oracle):
    """the gather of k_uri_lines: 64 heads in round 0; a lane of 66 blocks at
    0 / 31 / 63; a line's first block 63, 64, 65, 127, 128; BAD and '-'
    request lines at the edges and in runs before the line on block 64"""
    _all(oracle, uoc.block_cases())


def test_owner_blocks_overflow_gpu(oracle):
    """above the compact buffer: k_uri_overflow's gather, two batches of rounds"""
    c = uoc.block_overflow_case()
    r = decided(oracle, c)
    assert r.counters["ok"] == 64 and r.diag["uri_overflow_waves"] == 1, r.diag


# ------------------------------------------------------------------ events
@pytest.mark.parametrize("where", ["req", "ref", "both"])
def test_owner_events_gpu(oracle, where):
    """uri_walk_coop: the same arrangements in event space, the events in the
    request URI, the referer, or both"""
    _all(oracle, uoc.event_cases(where))


# ------------------------------------------------------------------ pieces
@pytest.mark.parametrize("named", [False, True], ids=["all", "named"])
def test_owner_pieces_gpu(oracle, named):
    """the spread piece pass: the same arrangements in piece space, with all
    paths and with one named parameter and a referer part"""
    _all(oracle, _pieces(), fields=uwc.NAMED_FIELDS if named else None)


def test_owner_pieces_three_formats_gpu(oracle):
    """the SLOT instance: the three-format handle, 'common' lines among the 'combined' ones"""
    _all(oracle, _pieces("mixed"))


def test_owner_pieces_direct_gpu(oracle):
    """LP_OPT_FORCE_DIRECT: every wave on k_uri_overflow's direct (HBM) path"""
    _all(oracle, _pieces(), options={lpa.OPT_FORCE_DIRECT: 1}, overflow=None)


# ------------------------------------------------------------------- reuse
def test_owner_reused_handle_gpu(oracle):
    """one handle: a pieces batch, a blocks batch, the pieces batch again (the
    head words and the arena hold the other batch's state in between)"""
    pieces = {c.name: c for c in _pieces()}["OP-first128"]
    blocks = {c.name: c for c in uoc.block_cases()}["OB-long0"]
    p = _parser(oracle, pieces)
    decided_with(oracle, pieces, p)
    decided_with(oracle, blocks, p)
    decided_with(oracle, pieces, p)
