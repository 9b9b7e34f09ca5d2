"""The straight-line first leaf of the fixed-shape instances on the GPU
(lp_device.h fixed_fast_leaf, parse_fixed.hip): the corpus of
fixed_fast_corpus.py line by line against the oracle through the fixed
instance, bit-equal to the run with LP_OPT_FIXED_SHAPE 0, at several chunk
sizes; waves whose lanes all take the fast leaf, all take the element walk, or
mix them; and the kernel's count of walked lines against the CPU unit's."""
import re

import numpy as np
import pytest

import fixed_fast_corpus as corpus
import fixed_fast_emu_lib as ff
import logparser_amd as lpa

pytestmark = pytest.mark.gpu

SHAPES = (("combined", 1), ("common", 2))
_PATHS, _ORACLE, _REF, _PARSERS, _FAST = {}, {}, {}, {}, {}


def paths(oracle, fmt):
    if fmt not in _PATHS:
        _PATHS[fmt] = oracle.possible_paths(fmt)
    return _PATHS[fmt]


def reference(oracle, fmt, line):
    """the oracle's (status, record) of a line, computed once"""
    key = (fmt, line)
    if key not in _REF:
        if fmt not in _ORACLE:
            _ORACLE[fmt] = oracle.Oracle(fmt, paths(oracle, fmt))
        _REF[key] = _ORACLE[fmt].parse_raw(line)
    return _REF[key]


def cpu_walked(fmt, lines):
    """lines the CPU unit's phase 1 sends through the element walk (flags bit 1)"""
    if fmt not in _FAST:
        _FAST[fmt] = ff.Fast(fmt)
    n, st, flags, first = _FAST[fmt].run(lines)
    assert n == 0, first
    return int(((flags >> 1) & 1).sum()), flags


def parse(oracle, fmt, data, options=None):
    # one handle per (format, options), kept for the module
    key = (fmt, tuple(sorted((options or {}).items())))
    if key not in _PARSERS:
        _PARSERS[key] = lpa.HttpdLoglineParser(fmt, paths(oracle, fmt), options=options)
    p = _PARSERS[key]
    r = p.parse_batch(data)
    buf, res = r.copy_to_host(with_input=False)
    cols = {k: v.copy() for k, v in r.columns(res).items()}
    return p, r, cols


def check(oracle, fmt, shape, lines, options=None, want_ok=0):
    """the lines through the fixed instance and through the generic one: the
    same bits; the fixed one's lines against the oracle.  Returns the fixed
    run's result."""
    data = b"".join(l + b"\n" for l in lines)
    off = dict(options or {})
    off[lpa.OPT_FIXED_SHAPE] = 0
    pf, rf, cf = parse(oracle, fmt, data, options)
    pg, rg, cg = parse(oracle, fmt, data, off)
    assert rf.diag["fixed_shape"] == shape and rg.diag["fixed_shape"] == 0, (rf.diag, rg.diag)
    assert rg.diag["walk_lines"] == 0, rg.diag   # (only a fixed-shape instance counts them)
    assert rf.n_lines == rg.n_lines == len(lines)
    assert rf.counters == rg.counters
    for k in ("overflow_waves", "deferred_chunks", "dfs_lines", "uri_repair_lines", "arena_ovf"):
        assert rf.diag[k] == rg.diag[k], (k, rf.diag, rg.diag)
    assert (rf.status == rg.status).all()
    assert sorted(cf) == sorted(cg)
    live = rf.status == lpa.LINE_OK
    for k in sorted(cf):
        # not compared bit by bit: arena_base (handed out by atomics, in
        # scheduling order) and the query tables' words (written only for a
        # URI that has a query; the records below read them)
        if k[0] == "arena_base" or k[0].startswith("q_"):
            continue
        a, b = cf[k][: rf.n_lines], cg[k][: rf.n_lines]
        rows = live  # (a line that is not OK has no values)
        if k[0].startswith("u_") and k[0] != "u_flags":
            bit = 1 | {"u_path": 1 << 6, "u_query": 1 << 4, "u_frag": 1 << 5}.get(k[0], 0)
            rows = live & ((cf[("u_flags", k[1])][: rf.n_lines] & bit) == bit)
        if k[0] != "status":
            a, b = a[rows], b[rows]
        assert np.array_equal(a, b), k
    n_ok = 0
    for i, l in enumerate(lines):
        s2 = int(rf.status[i])
        if s2 == lpa.LINE_FALLBACK:
            continue
        s1, r1 = reference(oracle, fmt, l)
        assert s1 != oracle.UNSUPPORTED and s1 == s2, (i, l[:300], s1, s2)
        if s1 == oracle.OK:
            assert rf.record_json(i) == r1, (i, l[:300])
            n_ok += 1
    assert n_ok >= want_ok, (n_ok, want_ok)
    return rf


@pytest.mark.parametrize("chunk_lines", [1, 17, 64, None], ids=["chunk1", "chunk17", "chunk64", "default"])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_corpus(oracle, name, shape, chunk_lines):
    lines = corpus.lines(name)
    options = {lpa.OPT_CHUNK_LINES: chunk_lines} if chunk_lines else None
    r = check(oracle, name, shape, lines, options=options, want_ok=len(lines) // 8)
    # the kernel counts a walked line only where the chunk kernel itself runs
    # phase 1 on it (not a line past its chunk's 64th or longer than the window)
    walked, _ = cpu_walked(name, lines)
    assert 0 < r.diag["walk_lines"] <= walked, (r.diag, walked)


@pytest.fixture(scope="module")
def base_lines():
    return lpa.synth(lpa.SYNTH_COMBINED, 20261022, 0, 2048).split(b"\n")[:-1]


def to_common(line):
    return line.rsplit(b' "', 2)[0]


def walker(name, line):
    """the same line with a %b longer than the fast digit test: it takes the
    element walk and stays OK"""
    big = b"1" * (corpus.DIGITS + 1)
    if name == "combined":
        out, k = re.subn(rb'(" \d{3}) (?:\d+|-) "', rb'\1 ' + big + b' "', line, count=1)
    else:
        out, k = re.subn(rb'(" \d{3}) (?:\d+|-)$', rb'\1 ' + big, line, count=1)
    assert k == 1, line
    return out


@pytest.mark.parametrize("every", [0, 1, 2, 7, 64, 65], ids=["all-fast", "all-walk", "every2", "every7", "every64", "every65"])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_wave_patterns(oracle, base_lines, name, shape, every):
    """every k-th line takes the element walk (0: none), so waves hold only
    fast lanes, only walking lanes, or both; the kernel's count is the CPU's"""
    lines = base_lines if name == "combined" else [to_common(l) for l in base_lines]
    lines = [walker(name, l) if every and i % every == 0 else l for i, l in enumerate(lines)]
    want = len(range(0, len(lines), every)) if every else 0
    walked, flags = cpu_walked(name, lines)
    assert walked == want, (walked, want)
    r = check(oracle, name, shape, lines, want_ok=len(lines))
    assert r.diag["walk_lines"] == walked, (r.diag, walked)
    assert r.diag["dfs_lines"] == 0, r.diag
