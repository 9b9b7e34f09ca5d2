"""Predicate row selection, GPU part: lp_result_select_where on a device view
(where.hip's k_where_eval, then select.hip's compaction of its bits).  Every
expectation is where_corpus.expected_rows over the HOST-COPY table (table_from:
pinned against the oracle by test_gpu_parity / test_value_edges_gpu); the
device row list must equal it byte for byte, and so must select_where_from on
the host copy.  The CPU part is test_select_where.py.

The compaction's tiles in lines (csrc/kernels.h): a lane takes 16, a wave W =
SEL_WAVE_LINES = 1024, a block B = SEL_BLOCK_LINES = 4096; k_where_eval's wave
takes 64 lines, its block 256.

No case uses an out-of-range index or pointer: the error cases are refused by
the host's checks before anything is launched."""
import ctypes
import functools

import numpy as np
import pytest

import logparser_amd as lpa
import row_select_corpus as rsc
import where_corpus as wc
from where_corpus import BYTES, BYTESCLF, DATE, EPOCH, PATH, QP, QUERY, REFERER, STATUS, UA

pytestmark = pytest.mark.gpu

W, B = lpa.SEL_WAVE_LINES, lpa.SEL_BLOCK_LINES
Wh = lpa.Where
EQ, LT, LE, GT, GE, BETWEEN = lpa.WHERE_EQ, lpa.WHERE_LT, lpa.WHERE_LE, lpa.WHERE_GT, lpa.WHERE_GE, lpa.WHERE_BETWEEN
PREFIX, SUFFIX, CONTAINS, IS_NULL = lpa.WHERE_PREFIX, lpa.WHERE_SUFFIX, lpa.WHERE_CONTAINS, lpa.WHERE_IS_NULL
STR_COLS = [(STATUS, str), (BYTESCLF, str), (EPOCH, str), (DATE, str), (PATH, str), (QP, str), (QUERY, str),
            (REFERER, str), (UA, str), ("@line", str)]
INT_COLS = [(BYTESCLF, int), (BYTES, int), (EPOCH, int), ("@offset", int), ("@lineno", int), ("@status", int)]


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _new_parser(fmt="combined"):
    """every path of the format and the request's query wildcard"""
    return lpa.HttpdLoglineParser(fmt, [f for f in lpa.get_possible_paths(fmt) if not f.endswith("*")] + [wc.QWILD])


@functools.lru_cache(None)
def _parser(fmt="combined"):
    """one handle per LogFormat for the tests that parse their own batch (a batch lives until the handle's next)"""
    return _new_parser(fmt)


class Batch:
    """a parsed batch, its host copy and the host copy's decoded table columns (built once per column set)"""

    def __init__(self, lines_status, data=None, parser=None):
        lines = [l for l, _ in lines_status]
        self.r = (parser or _parser()).parse_batch(rsc.join_lf(lines) if data is None else data)
        assert self.r.n_lines == len(lines)
        assert self.r.status.tolist() == [s for _, s in lines_status]
        self.buf, self.res = self.r.copy_to_host()
        self.table = {}

    def need(self, terms):
        cols = sorted({(t.path, t.kind) for t in terms if (t.path, t.kind) not in self.table}, key=lambda c: c[0])
        for typ in (str, int):  # (one table per kind: a path may be taken as both)
            part = [c for c in cols if c[1] is typ]
            if part:
                self.table.update(wc.decoded(self.r.table_from(self.res, part, threads=4, decode=False), part))

    def check(self, terms, mask=lpa.SEL_OK, first=0, count=None):
        """select_where_device == expected_rows(the host copy's table) == select_where_from; returns the rows"""
        r = self.r
        count = r.n_lines - first if count is None else count
        self.need(terms)
        want = wc.expected_rows(self.table, r.status, first, count, mask, terms)
        got = r.select_where_device(terms, mask, first, count)
        assert got.is_cuda and str(got.dtype) == "torch.int64"
        assert _np(got).tobytes() == want.tobytes(), (r.n_lines, first, count, mask, terms, _np(got)[:8], want[:8])
        host = r.select_where_from(self.res, terms, mask, first, count)
        assert host.dtype == np.int64 and host.tobytes() == want.tobytes(), (r.n_lines, first, count, mask, terms, "host")
        return want


@functools.lru_cache(None)
def _planted():
    """the batch several tests share, on a handle of its own"""
    return Batch(wc.with_planted(300), parser=_new_parser())


# -------------------------------------------------------------- 1. tile edges
@pytest.mark.parametrize("n", (1, 15, 16, 17, 63, 64, 65, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1))
def test_tile_edges_gpu(n):
    """a predicate true on exactly one line at the tiles' edges, on every line, on none"""
    b = Batch(wc.lines(n))
    b.need([Wh(PATH, EQ, b""), Wh("@lineno", EQ, 0)])
    for at in sorted({0, n - 1} | {x for x in (15, 16, 63, 64) if x < n}):
        path, lineno = b.table[(PATH, str)][at], b.table[("@lineno", int)][at]
        assert b.check([Wh(PATH, EQ, path)]).tolist() == [at]
        if at in (0, n - 1, 63):  # the instance with pseudo-columns
            assert b.check([Wh("@lineno", EQ, lineno), Wh(PATH, EQ, b"nowhere")]).tolist() == [at]
    assert len(b.check([Wh(PATH, PREFIX, b"/")])) == n
    assert len(b.check([Wh(PATH, PREFIX, b"x")])) == 0


def test_windows_gpu():
    """first % 64 in 0, 1, 15, 16, 63 against counts around a lane's 16 lines, k_where_eval's wave of 64
    and the compaction's wave W; in the first block and across the second's start"""
    n = B + W + 57
    b = Batch(wc.lines(n, "mixed"))
    terms = [Wh(STATUS, EQ, "500"), Wh(STATUS, EQ, "502"), Wh("@status", EQ, rsc.FALLBACK)]
    for base in (0, B - 64):
        for f in (0, 1, 15, 16, 63):
            for count in (0, 15, 16, 17, 63, 64, 65, W - 1, W, W + 1):
                got = b.check(terms, mask=7, first=base + f, count=count)
                assert count < 15 or len(got) > 0
    for count in (1, 16, W + 1, n):  # windows that end at the batch's last line
        b.check(terms[:2], first=n - count, count=count)


# ------------------------------------------------------ 2. every op and kind
def _string_terms(path, v):
    """every STRING op on path, operands cut from the value v of one line; and the empty operand"""
    a = len(v) // 3
    ops = [(EQ, v), (PREFIX, v[:a + 1]), (SUFFIX, v[-(a + 1):]), (CONTAINS, v[a:2 * a + 1]), (EQ, v + b"x"),
           (PREFIX, v + b"x"), (SUFFIX, b"x" + v), (CONTAINS, v[:-1] + b"\x01"), (EQ, b""), (PREFIX, b""), (SUFFIX, b""),
           (CONTAINS, b"")]
    return [Wh(path, op, o) for op, o in ops] + [Wh(path, IS_NULL, kind=str)]


def _long_terms(path, x):
    ops = [(EQ, x, None), (LT, x, None), (LE, x, None), (GT, x, None), (GE, x, None), (BETWEEN, x - 40, x + 40),
           (BETWEEN, x, x), (BETWEEN, x + 1, x - 1), (EQ, -2 ** 63, None), (LE, 2 ** 63 - 1, None)]
    return [Wh(path, op, lo, hi) for op, lo, hi in ops] + [Wh(path, IS_NULL, kind=int)]


@pytest.mark.parametrize("col", STR_COLS + INT_COLS, ids=lambda c: "%s-%s" % (c[0], c[1].__name__))
def test_every_op_and_kind_gpu(col):
    """each op, plain and negated, on a token as LONG / STRING, a converter, a time field as LONG and as
    formatted STRING, a URI part from the arena, a query parameter, the raw query string with its '&',
    a long taken as STRING, and the four pseudo-columns; under the OK mask and under every status"""
    b = _planted()
    path, kind = col
    b.need([Wh(path, IS_NULL, kind=kind)])
    vals = b.table[col]
    ok = [i for i in range(b.r.n_lines) if b.r.status[i] == 0 and vals[i] is not None]
    assert len(ok) > 100
    for at in (ok[7], ok[-1]):
        v = vals[at]
        if path == QUERY:
            assert v[:1] == b"&"  # the raw query string has its leading '&'
        for t in (_string_terms(path, v) if kind is str else _long_terms(path, v)):
            for neg in (False, True):
                term = Wh(t.path, t.op, t.value, t.hi, kind=kind, negate=neg)
                for mask in (lpa.SEL_OK, 7):
                    got = b.check([term], mask=mask)
                    if not neg and t.op == EQ and t.value == v:
                        assert at in got.tolist()


def test_null_against_zero_gpu():
    """%b "-": the BYTESCLF token is null, the BYTES converter 0; a "-" referer is null; an absent parameter is
    null, an empty one the empty string"""
    b = _planted()
    dash = b.check([Wh(BYTESCLF, IS_NULL, kind=int)])
    assert len(dash) > 20 and b.check([Wh(BYTES, EQ, 0), Wh(BYTESCLF, IS_NULL, kind=int, group=1)]).tolist() == dash.tolist()
    assert len(b.check([Wh(BYTES, IS_NULL, kind=int)])) == 0
    assert len(b.check([Wh(BYTESCLF, EQ, 0)])) > 20
    assert len(b.check([Wh(REFERER, IS_NULL, kind=str)])) > 20
    absent, empty = b.check([Wh(QP, IS_NULL, kind=str)]), b.check([Wh(QP, EQ, b"")])
    assert len(absent) > 20 and len(empty) > 20 and not set(absent.tolist()) & set(empty.tolist())
    assert len(b.check([Wh(QP, PREFIX, b"w")])) > 20 and len(b.check([Wh(QP, EQ, b"first")])) == 0  # the last wins
    assert len(b.check([Wh(BYTESCLF, PREFIX, "1")])) > 20  # a STRING taken from a long: its decimal text


def test_raw_line_search_gpu():
    """"@line" CONTAINS over the FALLBACK lines: the line longer than 8191 bytes, the one with invalid UTF-8"""
    b = _planted()
    fb = lpa.SEL_FALLBACK
    long_line = b.check([Wh("@line", CONTAINS, b"x" * 255)], mask=7)
    assert long_line.tolist() == [300 + 5]
    assert b.check([Wh("@line", CONTAINS, b"\xff\xfe\xc3(")], mask=7).tolist() == [300 + 9]
    assert b.check([Wh("@line", SUFFIX, b"\xc3(\"")], mask=fb).tolist() == [300 + 9]
    marked = b.check([Wh("@line", CONTAINS, b"ua\x7f")], mask=7)
    assert marked.tolist() == rsc.expected_rows(b.r.status, 0, b.r.n_lines, fb).tolist()
    assert len(b.check([Wh("@line", CONTAINS, b"ua\x7f")])) == 0  # (no OK line holds it)
    assert b.check([Wh("@line", EQ, b"")], mask=7).tolist() == [300 + 11]  # the empty line: not null
    assert b.check([Wh("@line", EQ, b"garbage")], mask=lpa.SEL_BAD).tolist() == \
        [i for i, (l, _) in enumerate(wc.with_planted(300)) if l == b"garbage"]


# ------------------------------------------------------------------ 3. groups
def test_groups_gpu():
    b = Batch(wc.lines(B + 300, "mixed"))
    n = b.r.n_lines
    f = [wc.field(k) for k in range(n)]
    ok = [k for k in range(n) if b.r.status[k] == 0]
    assert b.check([Wh(STATUS, EQ, "503")]).tolist() == [k for k in ok if f[k]["status"] == 503]
    two = [Wh(STATUS, EQ, "500"), Wh(PATH, PREFIX, b"/api/", group=1)]
    assert b.check(two).tolist() == [k for k in ok if f[k]["status"] == 500 and f[k]["path"].startswith(b"/api/")]
    # status IN {500, 502, 503} AND the path under /api/ AND NOT the user agent contains "bot"
    terms = [Wh(STATUS, EQ, s, group=0) for s in ("500", "502", "503")] + \
        [Wh(PATH, PREFIX, b"/api/", group=1), Wh(UA, CONTAINS, wc.MARK, group=2, negate=True)]
    want = [k for k in ok if f[k]["status"] in (500, 502, 503) and f[k]["path"].startswith(b"/api/")
            and wc.MARK not in f[k]["ua"]]
    assert len(want) > 50 and b.check(terms).tolist() == want
    # eight terms: six OR-ed, two more groups
    eight = [Wh(STATUS, EQ, str(s), group=1) for s in wc.STATUSES] + \
        [Wh(BYTESCLF, IS_NULL, kind=int, group=4, negate=True), Wh(REFERER, CONTAINS, b"?x=", group=7)]
    assert b.check(eight).tolist() == [k for k in ok if f[k]["bytes"] is not None and f[k]["referer"] is not None]
    # a first group false on every line: every wave skips the rest
    assert len(b.check([Wh(PATH, PREFIX, b"nowhere", group=0)] + [Wh(UA, CONTAINS, b"o", group=1 + g) for g in range(7)])) == 0
    # ... false on all but one wave's line
    one = [Wh(PATH, EQ, f[ok[-1]]["path"], group=0), Wh(UA, CONTAINS, b"", group=1), Wh("@line", CONTAINS, b"HTTP/1.1", group=2)]
    assert b.check(one).tolist() == [ok[-1]]


# -------------------------------------------------------- 4. status interplay
def test_status_interplay_gpu():
    b = _planted()
    r = b.r
    for mask in range(1, 8):
        null = b.check([Wh(REFERER, IS_NULL, kind=str)], mask=mask)
        not_ok = [i for i in range(r.n_lines) if r.status[i] != 0 and (mask >> r.status[i]) & 1]
        assert set(not_ok) <= set(null.tolist())  # a BAD / FALLBACK line has only null values
        assert not set(b.check([Wh(REFERER, IS_NULL, kind=str, negate=True)], mask=mask).tolist()) & set(not_ok)
        big = b.check([Wh(BYTESCLF, GE, 500)], mask=mask)
        assert all(r.status[i] == 0 for i in big)
        assert set(not_ok) <= set(b.check([Wh(BYTESCLF, GE, 500, negate=True)], mask=mask).tolist())
        assert b.check([Wh("@status", EQ, rsc.BAD)], mask=mask).tolist() == \
            (rsc.expected_rows(r.status, 0, r.n_lines, lpa.SEL_BAD).tolist() if mask & lpa.SEL_BAD else [])
        # no terms: what lp_result_select selects
        assert _np(r.select_where_device([], mask)).tobytes() == _np(r.select_device(mask)).tobytes() == \
            r.select_where_from(b.res, [], mask).tobytes() == rsc.expected_rows(r.status, 0, r.n_lines, mask).tobytes()
    assert len(r.select_where_device([Wh(PATH, PREFIX, b"/")], 0)) == 0  # mask 0 selects nothing


# ------------------------------------------------------- 5. several LogFormats
def test_several_logformats_gpu():
    """combined and common lines interleaved: a user-agent term is null on a common line"""
    n = 333
    ls = [(wc.common_line(k), 0) if k % 3 == 1 else (wc.ok_line(k), 0) for k in range(n)]
    b = Batch(ls, parser=_parser("combined\ncommon"))
    common = [k for k in range(n) if k % 3 == 1]
    assert b.check([Wh(UA, IS_NULL, kind=str)]).tolist() == common
    assert b.check([Wh(UA, CONTAINS, b"", negate=True)]).tolist() == common
    bots = b.check([Wh(UA, CONTAINS, wc.MARK)]).tolist()
    assert bots == [k for k in range(n) if k % 3 != 1 and wc.MARK in wc.field(k)["ua"]] and len(bots) > 50
    both = b.check([Wh(STATUS, EQ, "404"), Wh(UA, PREFIX, b"curl", group=1, negate=True)]).tolist()
    assert both == [k for k in range(n) if wc.field(k)["status"] == 404 and (k % 3 == 1 or not wc.field(k)["ua"].startswith(b"curl"))]
    b.check([Wh(PATH, PREFIX, b"/static/"), Wh(UA, SUFFIX, wc.MARK), Wh(BYTESCLF, BETWEEN, 100, 300, group=1)])


# -------------------------------------------------- 6. last bytes of the buffer
def test_last_bytes_of_the_buffer_gpu():
    """an unterminated final line, the input a device tensor exactly as long as the data: the line's and the
    last field's final bytes are compared where they end the buffer (or one byte before its end)"""
    import torch
    for n in (1, 67):
        ls = wc.lines(n)
        data = rsc.join_lf([l for l, _ in ls])[:-1]
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        assert t.numel() == len(data)
        b = Batch(ls, data=t)
        last, ua = ls[-1][0], wc.field(n - 1)["ua"]
        for terms, hit in (([Wh("@line", SUFFIX, last[-9:])], True), ([Wh("@line", EQ, last)], True),
                           ([Wh("@line", CONTAINS, last[-3:])], True), ([Wh("@line", SUFFIX, last[-9:] + b"\"")], False),
                           ([Wh("@line", EQ, last + b"\x00")], False), ([Wh(UA, SUFFIX, ua[-5:])], True),
                           ([Wh(UA, EQ, ua)], True), ([Wh(UA, CONTAINS, ua[-2:])], True), ([Wh(UA, SUFFIX, ua[-5:] + b"\"")], False),
                           ([Wh(UA, CONTAINS, ua[-2:] + b"\"")], False)):
            got = b.check(terms).tolist()
            assert (n - 1 in got) == hit, terms


# ------------------------------------------------- 7. size protocol and errors
def _term(path, kind, op, group=0, lo=0, hi=0, s=None, str_len=None):
    t = lpa.LpWhereTerm()
    t.path = path.encode() if path is not None else None
    t.kind, t.op, t.group, t.lo, t.hi = kind, op, group, lo, hi
    t.str = s
    t.str_len = (len(s) if s is not None else 0) if str_len is None else str_len
    return t


def _raw(b, on_host, terms, n_terms=None, mask=lpa.SEL_OK, cap=0, first=0, count=None):
    """one lp_result_select_where into a buffer of cap + 8 int64 words, every byte 0x5A: (rc, rows_len, the buffer)"""
    import torch
    r = b.r
    if on_host:
        res = b.res
        buf = np.full(8 * (cap + 8), 0x5A, dtype=np.uint8).view(np.int64)
        ptr = buf.ctypes.data
    else:
        res = lpa.LpResult()
        assert lpa.lib().lp_result_view(r._p._h, ctypes.byref(res)) == lpa.LP_OK
        buf = torch.full((8 * (cap + 8),), 0x5A, dtype=torch.uint8, device="cuda").view(torch.int64)
        ptr = buf.data_ptr()
    arr = (lpa.LpWhereTerm * max(1, len(terms)))(*terms)
    n = ctypes.c_uint64(12345)
    rc = lpa.lib().lp_result_select_where(r._p._h, ctypes.byref(res), first, r.n_lines - first if count is None else count,
                                          mask, arr, len(terms) if n_terms is None else n_terms, ptr, cap, ctypes.byref(n))
    return rc, int(n.value), _np(buf)


@pytest.mark.parametrize("on_host", [False, True])
def test_size_protocol_and_errors_gpu(on_host):
    b = _planted()
    S, L = lpa.CAST_STRING, lpa.CAST_LONG
    terms = [_term(PATH, S, PREFIX, s=b"/api/"), _term(BYTESCLF, L, GE, lo=0, group=1)]
    want = b.check([Wh(PATH, PREFIX, b"/api/"), Wh(BYTESCLF, GE, 0, group=1)])
    need = len(want)
    assert need > 16  # (more rows than one lane's 16-line group holds)
    sentinel = np.full(8, 0x5A, dtype=np.uint8).view(np.int64)[0]
    for cap in (0, need - 1):
        rc, n, buf = _raw(b, on_host, terms, cap=cap)
        assert rc == lpa.LP_E_NOMEM and n == need, (cap, rc, n, need)
        assert (buf == sentinel).all(), cap  # nothing written, below the capacity or past it
    rc, n, buf = _raw(b, on_host, terms, cap=need)
    assert rc == lpa.LP_OK and n == need
    assert buf[:need].tobytes() == want.tobytes() and (buf[need:] == sentinel).all()
    rc, n, buf = _raw(b, on_host, terms, mask=0, cap=4)  # mask 0 selects nothing
    assert rc == lpa.LP_OK and n == 0 and (buf == sentinel).all()
    big = b"y" * 255
    invalid = {
        "n_terms 9": ([terms[0]] * 9, None), "n_terms -1": (terms, -1),
        "null path": ([_term(None, S, EQ, s=b"x")], None),
        "kind DOUBLE": ([_term(BYTESCLF, lpa.CAST_DOUBLE, EQ)], None), "kind 0": ([_term(PATH, 0, EQ, s=b"x")], None),
        "kind both": ([_term(BYTESCLF, S | L, EQ)], None),
        "casts lack LONG": ([_term(STATUS, L, EQ, lo=500)], None), "casts lack LONG (date)": ([_term(DATE, L, EQ)], None),
        "@line as LONG": ([_term("@line", L, EQ)], None), "@offset as STRING": ([_term("@offset", S, EQ, s=b"0")], None),
        "op 10": ([_term(PATH, S, 10, s=b"x")], None), "op -1": ([_term(PATH, S, -1, s=b"x")], None),
        "op bit": ([_term(PATH, S, EQ | 0x200, s=b"x")], None),
        "PREFIX on LONG": ([_term(BYTESCLF, L, PREFIX, s=b"1")], None), "LT on STRING": ([_term(PATH, S, LT, s=b"x")], None),
        "BETWEEN on STRING": ([_term(PATH, S, BETWEEN, s=b"x")], None),
        "group decreases": ([_term(PATH, S, EQ, group=1, s=b"x"), _term(PATH, S, EQ, group=0, s=b"x")], None),
        "str_len 256": ([_term(PATH, S, EQ, s=big + b"y")], None), "str_len -1": ([_term(PATH, S, EQ, s=b"x", str_len=-1)], None),
        "null str": ([_term(PATH, S, EQ, s=None, str_len=3)], None),
        "pool": ([_term(QP, S, CONTAINS, s=big)] * 8, None),  # 8 x (the name "k7" + 255 bytes) > 2048
        "mask bit": (terms, None, 8),
    }
    for what, case in invalid.items():
        rc, n, buf = _raw(b, on_host, case[0], n_terms=case[1], cap=4, mask=case[2] if len(case) > 2 else lpa.SEL_OK)
        assert rc == lpa.LP_E_INVALID and (buf == sentinel).all(), (what, rc)
    assert _raw(b, on_host, [_term(PATH, S, CONTAINS, s=big)] * 8, cap=4)[0] == lpa.LP_OK  # 2040 bytes fit
    for path in ("STRING:no.such.path", "HTTP.PATH:request.firstline.uri.pathx", "nocolon"):
        assert _raw(b, on_host, [_term(path, S, EQ, s=b"x")], cap=4)[0] == lpa.LP_E_MISSING, path
    assert _raw(b, on_host, terms, cap=4, first=b.r.n_lines, count=1)[0] == lpa.LP_E_INVALID  # past the batch
    assert _raw(b, on_host, terms, cap=4, first=-1, count=1)[0] == lpa.LP_E_INVALID
    assert _raw(b, on_host, terms, cap=4, first=0, count=-1)[0] == lpa.LP_E_INVALID
    # the Python mirror's exceptions
    with pytest.raises(lpa.MissingDissectorsException):
        b.r.select_where_device([Wh("STRING:no.such.path", EQ, "x")])
    with pytest.raises(ValueError):
        b.r.select_where_device([Wh(STATUS, GE, 500)])


def test_timing_gpu():
    b = _planted()
    b.r.select_where_device([Wh(UA, CONTAINS, wc.MARK)])
    pred, compact = b.r.select_where_timing()
    assert pred > 0 and compact > 0
    t = (ctypes.c_float * 20)(*([-1.0] * 20))
    assert lpa.lib().lp_last_timing(b.r._p._h, t, 18) == 18 and t[18] == -1.0  # a caller of 18 sees what it always saw
    assert lpa.lib().lp_last_timing(b.r._p._h, t, 20) == 20 and t[18] == pytest.approx(pred) and t[19] == pytest.approx(compact)


# ----------------------------------------------------------------- 8. hand-on
def test_hand_on_to_the_dense_table_gpu():
    """table_device(cols, rows=select_where_device(...)) == the gather of the whole-batch device table"""
    b = Batch(wc.lines(W + 200, "mixed"))
    terms = [Wh(STATUS, PREFIX, "5"), Wh(PATH, PREFIX, b"/api/", group=1)]
    want = b.check(terms)
    assert len(want) > 50
    cols = [(PATH, str), (EPOCH, int), (UA, str), ("@lineno", int)]
    rows = b.r.select_where_device(terms)
    dense, whole = b.r.table_device(cols, rows=rows), b.r.table_device(cols)
    for path, typ in cols:
        (dv, dok), (wv, wok) = dense[path], whole[path]
        wok = _np(wok)
        assert _np(dok).tolist() == wok[want].tolist() and _np(dok).all(), path
        if typ is str:
            off, chars, _ = rsc.gather_arrow(_np(wv[0]), _np(wv[1]), wok, want)
            assert _np(dv[0]).tobytes() == off.tobytes() and _np(dv[1])[:off[-1]].tobytes() == chars.tobytes(), path
        else:
            assert _np(dv).tobytes() == _np(wv)[want].tobytes(), path


# -------------------------------------------------- 9. existing select unchanged
def test_status_select_unchanged_gpu():
    """the status-only select after the compaction kernels took their match-word source as a parameter"""
    ls = rsc.pattern_lines(2 * B + 1, "mixed")
    p = lpa.HttpdLoglineParser(rsc.FMT, [f for f in lpa.get_possible_paths(rsc.FMT) if not f.endswith("*")])
    r = p.parse_batch(rsc.join_lf([l for l, _ in ls]))
    assert r.status.tolist() == [s for _, s in ls]
    for mask in range(8):
        assert _np(r.select_device(mask)).tobytes() == rsc.expected_rows(r.status, 0, r.n_lines, mask).tobytes(), mask
    for first, count in ((1, B), (15, 2 * B - 30), (B + 17, 33), (2 * B, 1)):
        assert _np(r.select_device(7 & ~lpa.SEL_BAD, first, count)).tobytes() == \
            rsc.expected_rows(r.status, first, count, 7 & ~lpa.SEL_BAD).tobytes(), (first, count)
