"""The LogFormat matcher against an independent regex engine, GPU part: the corpora of regex_corpus.py through
HttpdLoglineParser.parse_batch, every line's status and record against Python's `re` (regex_ref.py), one handle
and one batch of a few thousand lines per format.  The kernel instances and passes the lines can take are each
made to take them: the fixed-shape and the per-class instances of the chunk kernel, the literal-aware and the
several-format instance, the queued-line kernels (lines that need the DFS; chunks of more than 64 lines), the
deferred pass and the direct-HBM path.  The CPU part (oracle and emulation against `re`, what the corpora must
hold) is test_regex_priority.py.
"""
import pytest

import emu_lib
import logparser_amd as lpa
import regex_ref as rr
from test_regex_priority import STAGES, check

pytestmark = pytest.mark.gpu

assert (lpa.LINE_OK, lpa.LINE_BAD, lpa.LINE_FALLBACK) == (0, 1, 2)  # check()'s codes

_EMU_FALLBACK = {}


def emu_fallback(c, key, fields, lines):
    """the lines the CPU emulation of the same device code leaves undecided (computed once per batch)"""
    if key not in _EMU_FALLBACK:
        emu_lib.lib().emu_set_masks(1)
        e = emu_lib.Emu(c.logformat, fields)
        assert e.status == 0, e.err
        _EMU_FALLBACK[key] = [i for i, l in enumerate(lines) if e.parse_raw(l)[0] == 2]
    return _EMU_FALLBACK[key]


def run(oracle, name, options=None, extra=(), stages=False):
    """the handle's corpus (plus the `extra` lines) as one batch: every line against `re` (no match <=> BAD,
    match => OK with every group's text), FALLBACK on exactly the emulation's lines.  stages: STAGES requested
    too (common / combined: the program of the fixed-shape instances)"""
    c = rr.case(oracle, name)
    fields = c.fields + (STAGES if stages else [])
    lines, want = c.lines, c.want
    if extra:
        lines = lines + list(extra)
        want = want + [c.expect(l) for l in extra]
    p = lpa.HttpdLoglineParser(c.logformat, fields, options=options)
    r = p.parse_batch(b"".join(l + b"\n" for l in lines))
    assert r.n_lines == len(lines)
    fb = []
    for i, (l, w) in enumerate(zip(lines, want)):
        st = int(r.status[i])
        if check(c, i, l, w, st, r.record_json(i) if st == lpa.LINE_OK else None, exact=False, more=stages):
            fb.append(i)
    assert fb == emu_fallback(c, (name, len(lines), stages), fields, lines)
    assert r.counters["fallback"] == len(fb) <= 0.02 * len(lines)
    assert r.counters["bad"] == sum(w is None for i, w in enumerate(want) if i not in set(fb))
    return r


@pytest.mark.parametrize("name", rr.NAMES)
def test_gpu_against_re(oracle, name):
    """exactly the groups' paths requested: the chunk kernel's instance of the program's class (SIMPLE for the
    Apache family, the literal-aware and the several-format one), the queued-line kernels for the DFS"""
    r = run(oracle, name)
    assert r.diag["dfs_lines"] > 0, r.diag  # lines that needed the backtracking DFS (k_parse_ovf_lines / k_route_ovf)
    assert r.diag["fixed_shape"] == 0, r.diag


@pytest.mark.parametrize("name", ["combined", "common"])
@pytest.mark.parametrize("fixed", [1, 0])
def test_fixed_shape_instance_gpu(oracle, name, fixed):
    """common / combined with their time and first-line stages: the fixed-shape instance, and the same program
    with LP_OPT_FIXED_SHAPE 0 (the SIMPLE instance)"""
    r = run(oracle, name, {lpa.OPT_FIXED_SHAPE: fixed}, stages=True)
    assert (r.diag["fixed_shape"] != 0) == bool(fixed) and r.diag["dfs_lines"] > 0, r.diag


@pytest.mark.parametrize("name,wait", [("combined", -1), ("combined", -2), ("common", -1), ("nginx", -1)])
def test_deferred_pass_gpu(oracle, name, wait):
    """the chunk wait forced (LP_OPT_CHUNK_WAIT < 0): the deferred pass parses the same lines"""
    r = run(oracle, name, {lpa.OPT_CHUNK_WAIT: wait}, stages=name in ("combined", "common"))
    assert r.diag["deferred_chunks"] > 0 and r.diag["dfs_lines"] > 0, r.diag


@pytest.mark.parametrize("name", ["end_greedy", "nospace", "nospace+brackets"])
def test_overflow_lines_gpu(oracle, name):
    """the corpus followed by the shorter half of its short lines, six times over: a byte chunk sized for the
    batch's mean line then holds more than 64 of them, and its 65th line on goes to k_parse_ovf_lines (a
    several-format handle: routed by k_route_ovf first)"""
    c = rr.case(oracle, name)
    extra = sorted(c.short, key=len)[:len(c.short) // 2] * 6
    mean = (sum(map(len, c.lines + extra)) + len(c.lines + extra)) / len(c.lines + extra)
    # a chunk is sized for at most 54 lines of the batch's mean length (parse.hip): the short lines fit in it
    # 96 at a time and more, wherever its edges fall
    assert 54 * mean / (sum(map(len, extra)) / len(extra) + 1) > 96
    r = run(oracle, name, extra=extra)
    assert r.diag["overflow_waves"] > 0 and r.diag["dfs_lines"] > 0, r.diag


@pytest.mark.parametrize("name", ["combined", "nginx_tight"])
def test_direct_path_gpu(oracle, name):
    """LP_OPT_FORCE_DIRECT: the lines read from HBM with the SWAR scanners instead of the LDS window's masks"""
    run(oracle, name, {lpa.OPT_FORCE_DIRECT: 1}, stages=name == "combined")
