"""The separate line index (k_count_newlines, k_line_offsets) with no parse
behind it: a handle whose program is not on the device gets its lines from
the index alone and reports every one as FALLBACK.  And LP_OPT_ONE_PASS, which
once chose between that index and the chunk kernel for several LogFormats."""
import random

import pytest

import corpora
import logparser_amd as lpa
from test_gpu_parity import paths

pytestmark = pytest.mark.gpu

# the user agent captured twice: "the same output is produced by two tokens", a planner refusal
NOT_ON_DEVICE = '%h %l %u %t "%r" %>s %b "%{Referer}i" "%{User-Agent}i" "%{User-Agent}i"'


def hadoop_offsets(data):
    """line_off of a buffer, as the header states it: line i is
    data[off[i], off[i + 1] - 1) less the '\\r' of a "\\r\\n" terminator, so an
    entry is the byte after a terminator and the end entry is len(data) after
    a terminated last line, len(data) + 1 after one without terminator"""
    off, i, n = [0], 0, len(data)
    while i < n:
        c = data[i]
        if c == 0x0D and i + 1 < n and data[i + 1] == 0x0A:
            i += 1
        if c == 0x0A or c == 0x0D:
            off.append(i + 1)
        i += 1
    if off[-1] < n:
        off.append(n + 1)
    return off


def check_index(p, buf):
    want = corpora.split_hadoop(buf)
    off = hadoop_offsets(buf)
    assert len(off) == len(want) + 1
    for i, l in enumerate(want):  # (the two restatements agree)
        raw = buf[off[i]:off[i + 1] - 1]
        assert (raw[:-1] if raw.endswith(b"\r") else raw) == l, (buf[:80], i)
    r = p.parse_batch(buf)
    assert r.n_lines == len(want), (buf[:80], r.n_lines, len(want))
    assert (r.status == lpa.LINE_FALLBACK).all(), buf[:80]
    c = r.counters
    assert (c["lines"], c["ok"], c["bad"], c["fallback"]) == (len(want), 0, 0, len(want)), c
    assert r.diag["overflow_waves"] == 0, r.diag
    assert [r.line_offset(i) for i in range(r.n_lines + 1)] == off, buf[:80]


def test_line_index_without_parse_gpu():
    """One handle, many batches: about 200 KiB of mixed terminators (three
    64 KiB index chunks, no final terminator), the same with one, the 40
    terminator-corner buffers of test_crlf_terminators_gpu, and one line
    without terminator: the line count, every status FALLBACK and every
    line_offset(i), i in 0..n_lines, against the Python split."""
    lines = lpa.synth_combined(20261019, 0, 800).split(b"\n")[:-1]
    p = lpa.HttpdLoglineParser(NOT_ON_DEVICE, ["HTTP.USERAGENT:request.user-agent"])
    data = corpora.crlf_join(lines, 9)
    assert 3 * 65536 < len(data) < 4 * 65536 and data[-1:] not in (b"\n", b"\r")
    check_index(p, data)
    assert p.device_program_ok is False and "two tokens" in p.unsupported_reason
    check_index(p, data + b"\r\n")
    rng = random.Random(4)
    pieces = [b"\r", b"\n", b"\r\n", b"\r\r", b"\n\r", b"\r\n\r\n", b"-", b"x", lines[0], lines[1]]
    for t in range(40):
        check_index(p, b"".join(rng.choice(pieces) for _ in range(rng.randrange(1, 30))))
    check_index(p, lines[2])
    check_index(p, data)  # (after smaller batches: the buffers are reused)


def test_one_pass_option_gpu(oracle):
    """LP_OPT_ONE_PASS is reserved: 1 is accepted and changes nothing, 0 (the
    removed line-index parse of several LogFormats) is LP_E_INVALID, which the
    Python layer raises as ValueError on first use."""
    from test_emu_parity import MIXED
    fields = paths(oracle, MIXED)
    p = lpa.HttpdLoglineParser(MIXED, fields)
    p._ensure()
    assert p.device_program_ok
    L = lpa.lib()
    assert L.lp_set_option(p._h, lpa.OPT_ONE_PASS, 1) == lpa.LP_OK
    assert L.lp_set_option(p._h, lpa.OPT_ONE_PASS, 0) == lpa.LP_E_INVALID
    assert L.lp_set_option(p._h, lpa.OPT_ONE_PASS, 2) == lpa.LP_E_INVALID
    lines = lpa.synth(lpa.SYNTH_MIXED, 20261018, 0, 256)
    r = p.parse_batch(lines)  # (the handle still parses after the refused value)
    assert r.n_lines == 256 and r.counters["ok"] == 256, r.counters
    q = lpa.HttpdLoglineParser(MIXED, fields, options={lpa.OPT_ONE_PASS: 0})
    with pytest.raises(ValueError):
        q.parse_batch(lines)
