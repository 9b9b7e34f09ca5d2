"""The chunk kernel's staging pass on the GPU (stage_chunk: one 64-byte mask
block per lane and round): the corpora of stage_block_corpus.py (checked on
the CPU by test_stage_block.py), every line against the oracle and the line
index against the byte-by-byte split, on every chunk instance and chunk
geometry."""
import pytest

import corpora
import logparser_amd as lpa
import stage_block_corpus as sb
from test_gpu_parity import gpu_vs_oracle, paths

pytestmark = pytest.mark.gpu

_PARSERS, _WANT = {}, {}
CHUNK_LINES = (1, 17, 50, 64)


@pytest.fixture(scope="module")
def base():
    return lpa.synth_combined(20261023, 0, 400).split(b"\n")[:-1]


def parser(fmt, fields, options=None):
    """one handle per (format, fields, options), kept for the module (a handle's
    first launch sets up its stream's scratch memory)"""
    key = (fmt, tuple(fields), tuple(sorted((options or {}).items())))
    if key not in _PARSERS:
        _PARSERS[key] = lpa.HttpdLoglineParser(fmt, list(fields), options=options)
    return _PARSERS[key]


def want_of(oracle, fmt, fields, data):
    """the oracle's (status, record) of every line of a batch, computed once"""
    key = (fmt, tuple(fields), data)
    if key not in _WANT:
        o = oracle.Oracle(fmt, fields)
        _WANT[key] = [o.parse_raw(l) for l in corpora.split_hadoop(data)]
    return _WANT[key]


def check(oracle, fmt, fields, data, options=None, stateless=True):
    """data through one handle: the line index against the byte-by-byte split,
    every line's status and record against the oracle (a FALLBACK line is the
    host's); stateless: the oracle's results may be shared between runs"""
    lines = corpora.split_hadoop(data)
    starts = sb.line_starts(data)
    assert len(starts) == len(lines)
    if options is None and not stateless:
        _, r = gpu_vs_oracle(oracle, fmt, fields, lines, data=data)
    else:
        r = parser(fmt, fields, options).parse_batch(data)
        assert r.n_lines == len(lines), (r.n_lines, len(lines), options)
        want = want_of(oracle, fmt, fields, data)
        n = {"ok": 0, "bad": 0, "fallback": 0}
        for i, (s1, r1) in enumerate(want):
            s2 = int(r.status[i])
            if s2 == lpa.LINE_FALLBACK:
                n["fallback"] += 1
                continue
            assert s1 != oracle.UNSUPPORTED, lines[i]
            assert s1 == s2, (i, lines[i], s1, s2, options)
            if s1 == oracle.OK:
                assert r1 == r.record_json(i), (i, lines[i], options)
                n["ok"] += 1
            else:
                n["bad"] += 1
        c = r.counters
        assert (c["lines"], c["ok"], c["bad"], c["fallback"]) == (len(lines), n["ok"], n["bad"], n["fallback"])
    got = [r.line_offset(i) for i in range(len(lines))]
    assert got == starts, next((i, a, b) for i, (a, b) in enumerate(zip(got, starts)) if a != b)
    if lines:
        assert r.line_offset(len(lines)) == (len(data) if data[-1:] in (b"\n", b"\r") else len(data) + 1)
    return r


def every_geometry(oracle, data):
    """the default geometry and LP_OPT_CHUNK_LINES 1, 17, 50, 64: each against
    the oracle (so equal to each other), statuses equal to the default run's"""
    fields = paths(oracle)
    r0 = check(oracle, "combined", fields, data)
    assert r0.diag["fixed_shape"] != 0
    for cl in CHUNK_LINES:
        r = check(oracle, "combined", fields, data, {lpa.OPT_CHUNK_LINES: cl})
        assert (r.status == r0.status).all() and r.counters == r0.counters, cl
    return r0


def test_start_residues(oracle, base):
    """line starts at every residue of a 64-byte block, a terminator in byte 63,
    lines across the 1 KiB DMA pieces and the 4 KiB rounds"""
    every_geometry(oracle, sb.residues(base))


def test_dense_starts_and_excess(oracle, base):
    """blocks with 1..64 starts (the rank's slow path up to plane 6), 64 x '\\n'
    aligned and not; more than 64 starts in a chunk: chunk_excess numbers what
    the staging pass counted (CHK_EXCESS would fail the batch)"""
    r = every_geometry(oracle, sb.dense_starts(base))
    assert r.diag["overflow_waves"] > 0, r.diag


def test_cr_terminators(oracle, base):
    """"\\r\\n" with the '\\r' in byte 15, 31, 47, 63 of a block, lone '\\r',
    "\\r\\r", '\\r' as the batch's last byte"""
    every_geometry(oracle, sb.crlf(base))


def test_chunk_boundaries(oracle, base):
    """a '\\n' at t_lo (= the chunk before's t_hi), at t_hi - 1 and in a chunk's
    first byte, whatever the chunk size"""
    data = sb.boundaries(base)
    every_geometry(oracle, data)
    # the deferred pass stages again: the same loop, every chunk
    r = check(oracle, "combined", paths(oracle), data, {lpa.OPT_CHUNK_WAIT: -1})
    nd = r.diag["deferred_chunks"]
    assert nd > 1 and sb.CB_MIN <= len(data) // nd and -(-len(data) // (nd - 1)) <= sb.CB_MAX, (nd, len(data))


def test_batch_ends(oracle, base):
    """a last line without a terminator; batches of fewer than 64 bytes, of
    exactly 1024 and 4096 bytes, and one whose last chunk is not whole KiB
    (plain loads instead of the LDS-DMA)"""
    fields = paths(oracle)
    body = b"".join(l + b"\n" for l in base[:40])
    cases = [b"\n".join(base[:30]),                     # unterminated, not whole KiB
             b"ab\ncd", b"\n", b"x", b"\r\n\r", b"a" * 63,  # fewer than 64 bytes
             body[:1023] + b"\n", body[:1024 - 7] + b"tail...",
             body[:4095] + b"\n", body[:4096 - 1] + b"\r",
             body[:4096 + 1024] + b"q",                 # whole KiB plus a piece
             body[:5000]]
    assert [len(c) for c in cases[6:10]] == [1024, 1024, 4096, 4096] and all(len(c) < 64 for c in cases[1:6])
    for data in cases:
        check(oracle, "combined", fields, data)
        check(oracle, "combined", fields, data, {lpa.OPT_CHUNK_LINES: 1})


def test_guard_bytes(oracle, base):
    """TAB and bytes >= 0x80 inside lines: windows that are not `clean`"""
    data = sb.guard_lines(base)
    r = every_geometry(oracle, data)
    assert r.counters["ok"] > 200, r.counters


@pytest.mark.parametrize("instance", ["fixed", "simple", "generic", "la", "mf"])
def test_every_instance(oracle, instance):
    """one corpus of real lines with the staging corners between them through
    each chunk instance: the fixed shape, SIMPLE (a field subset without the
    fixed instances), the generic one (config 3), the literal-aware one
    (config 4) and the several-format one (the three-format handle)"""
    wl = {"fixed": 2, "simple": 2, "generic": 3, "la": 4, "mf": 5}[instance]
    fmt = lpa.SYNTH_FORMATS[wl]
    lines = lpa.synth(wl, 20261024, 0, 1500).split(b"\n")[:-1]
    data = sb.mixed(lines, 40 + wl)
    options = None
    fields = paths(oracle, fmt)
    if instance == "simple":
        fields = ["IP:connection.client.host", "TIME.EPOCH:request.receive.time.epoch",
                  "HTTP.PATH:request.firstline.uri.path", "HTTP.USERAGENT:request.user-agent"]
        options = {lpa.OPT_FIXED_SHAPE: 0}
    r = check(oracle, fmt, fields, data, options, stateless=instance != "mf")
    assert (r.diag["fixed_shape"] != 0) == (instance == "fixed"), r.diag
    assert r.diag["overflow_waves"] > 0 and r.counters["ok"] >= 1300, (r.diag, r.counters)
