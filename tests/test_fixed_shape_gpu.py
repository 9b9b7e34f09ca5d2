"""The fixed-shape instances of the chunk parse kernel on the GPU (lp_fixed.h,
parse_fixed.hip): every batch is parsed by the shape's instance and again
with LP_OPT_FIXED_SHAPE 0 (the instances per program class); every SoA column
and counter must be bit-equal, and every line must equal the oracle."""
import numpy as np
import pytest

import corpora
import fixed_emu_lib as fx
import logparser_amd as lpa

pytestmark = pytest.mark.gpu

SHAPES = sorted(fx.SHAPES.items())
_PATHS, _ORACLE, _REF, _PARSERS = {}, {}, {}, {}


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


def to_common(line):
    return line.rsplit(b' "', 2)[0]


@pytest.fixture(scope="module")
def base_lines():
    return lpa.synth(lpa.SYNTH_COMBINED, 20261022, 0, 4096).split(b"\n")[:-1]


@pytest.fixture(scope="module")
def adv_sets():
    """the adversarial lines of each shape (this builds the CPU unit they come from)"""
    return {shape: fx.adversarial(shape) for _, shape in SHAPES}


def lines_of(name, lines):
    return lines if name == "combined" else [to_common(l) for l in lines]


def parse(oracle, fmt, data, options=None):
    # one handle per (format, options), kept for the module: a handle's first
    # launch of the queued-line kernels sets up its stream's scratch memory,
    # which takes longer than any batch here
    key = (fmt, tuple(sorted((options or {}).items())))
    if key not in _PARSERS:
        _PARSERS[key] = lpa.HttpdLoglineParser(fmt, paths(oracle, fmt), options=options)
    p = _PARSERS[key]
    r = p.parse_batch(data)
    buf, res = r.copy_to_host(with_input=False)
    cols = {k: v.copy() for k, v in r.columns(res).items()}
    return p, r, cols


def check(oracle, fmt, shape, lines, data=None, options=None, want_ok=None):
    """data (default: the lines, '\\n'-terminated) through the fixed instance and
    through the generic one: the same bits; the fixed one's lines against the
    oracle.  Returns the fixed run's result."""
    if data is None:
        data = b"".join(l + b"\n" for l in lines)
    off = dict(options or {})
    off[lpa.OPT_FIXED_SHAPE] = 0
    pf, rf, cf = parse(oracle, fmt, data, options)
    pg, rg, cg = parse(oracle, fmt, data, off)
    assert rf.diag["fixed_shape"] == shape and rg.diag["fixed_shape"] == 0, (rf.diag, rg.diag)
    assert rf.n_lines == rg.n_lines == len(lines)
    assert rf.counters == rg.counters
    for k in ("overflow_waves", "deferred_chunks", "dfs_lines", "uri_repair_lines", "arena_ovf"):
        assert rf.diag[k] == rg.diag[k], (k, rf.diag, rg.diag)
    assert (rf.status == rg.status).all()
    assert sorted(cf) == sorted(cg)
    live = rf.status == lpa.LINE_OK
    for k in sorted(cf):
        # not compared bit by bit: arena_base (the arena regions are handed out
        # by atomics, in scheduling order) and the query tables' words (written
        # only for a URI that has a query; the records below read them)
        if k[0] == "arena_base" or k[0].startswith("q_"):
            continue
        a, b = cf[k][: rf.n_lines], cg[k][: rf.n_lines]
        rows = live  # (a line that is not OK has no values)
        if k[0].startswith("u_") and k[0] != "u_flags":
            # (the URI kernel writes a URI's words only when it dissects it, UF_DONE,
            # and its path / query / fragment words only when the URI has one)
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
            assert rg.record_json(i) == r1, (i, l[:300])
            n_ok += 1
    if want_ok is not None:
        assert n_ok >= want_ok, (n_ok, want_ok)
    return rf


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
@pytest.mark.parametrize("name,shape", SHAPES)
def test_batches(oracle, base_lines, name, shape, n):
    check(oracle, name, shape, lines_of(name, base_lines[:n]), want_ok=n)


@pytest.mark.parametrize("name,shape", SHAPES)
def test_adversarial(oracle, adv_sets, name, shape):
    adv = adv_sets[shape]
    check(oracle, name, shape, adv, want_ok=len(adv) // 10)
    # ... each line at another offset of its window: the set rotated, a short line before it
    check(oracle, name, shape, [b"x" * 29] + adv[29:] + adv[:29], want_ok=len(adv) // 10)


@pytest.mark.parametrize("name,shape", SHAPES)
def test_chunk_geometry(oracle, base_lines, adv_sets, name, shape):
    """chunks of 3 lines; runs of very short lines, so that a chunk holds more
    than 64 lines; finished and deferred chunks side by side (CHUNK_WAIT -2)"""
    lines = lines_of(name, base_lines[:1500]) + adv_sets[shape][:200]
    check(oracle, name, shape, lines, options={lpa.OPT_CHUNK_LINES: 3}, want_ok=1500)
    short = []
    for i, l in enumerate(lines_of(name, base_lines[:1000])):
        short.append(l)
        if i % 100 == 7:
            short += [b"x", b"-"] * 100
    r = check(oracle, name, shape, short, want_ok=1000)
    assert r.diag["overflow_waves"] > 0, r.diag  # (lines past a chunk's 64th: k_parse_ovf_lines)
    r = check(oracle, name, shape, lines_of(name, base_lines), options={lpa.OPT_CHUNK_WAIT: -2}, want_ok=4096)
    assert r.diag["deferred_chunks"] > 0, r.diag


@pytest.mark.parametrize("name,shape", SHAPES)
def test_line_ends(oracle, base_lines, name, shape):
    """an unterminated last line; CRLF and lone-CR terminators"""
    lines = lines_of(name, base_lines[:300])
    check(oracle, name, shape, lines, data=b"\n".join(lines), want_ok=300)
    check(oracle, name, shape, lines[:1], data=lines[0] + b"\r\n", want_ok=1)
    data = corpora.crlf_join(lines, 3)
    assert corpora.split_hadoop(data) == lines
    check(oracle, name, shape, lines, data=data, want_ok=300)


def test_near_miss_runs_generic(oracle, base_lines):
    """one field more than combined: the generic instance, the same results"""
    fmt = '%h %l %u %t "%r" %>s %b "%{Referer}i" "%{User-Agent}i" %D'
    lines = [l + b" %d" % (i * 37) for i, l in enumerate(base_lines[:500])]
    r = check(oracle, fmt, 0, lines, want_ok=500)
    assert r.diag["fixed_shape"] == 0
