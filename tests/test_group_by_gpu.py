"""Grouped aggregates, GPU part: lp_result_group on a device view (group.hip's
k_group_insert, dict.hip's numbering, k_group_agg in both regimes).  Every
expectation is group_corpus.reference over the HOST-COPY table (table_from:
pinned against the oracle by test_gpu_parity / test_value_edges_gpu); the
device's rep, group_of and every value / valid must equal it byte for byte, and
so must group_from on the host copy.  The CPU part is test_group_by.py.

The kernels' tiles: a wave takes 64 rows, a block 256; k_group_agg's grid
stops at 1024 blocks, far above these shapes, so "several blocks" is n > 256.
The accumulation is privatised in LDS when groups x words <= the budget
(OPT_GROUP_LDS_WORDS, default 4096 words), else direct with the wave peel
(OPT_GROUP_PEEL rounds); every shape below runs in both.

No case uses an out-of-range index or pointer on the device: those are refused
by the host's checks before anything is launched, and their codes are asserted
on the host path."""
import ctypes
import functools

import numpy as np
import pytest

import group_corpus as gc
import logparser_amd as lpa
import row_select_corpus as rsc
import where_corpus as wc
from group_corpus import BYTES, BYTESCLF, DATE, EPOCH, METHOD, PATH, QP, STATUS

pytestmark = pytest.mark.gpu

A = lpa.Agg
ROWS, CNT, SUM, MIN, MAX = lpa.AGG_COUNT_ROWS, lpa.AGG_COUNT, lpa.AGG_SUM, lpa.AGG_MIN, lpa.AGG_MAX
BASIC = [A(ROWS), A(SUM, BYTES)]  # three words per group
FULL = [A(ROWS), A(SUM, BYTES), A(MIN, BYTES), A(MAX, BYTES), A(CNT, BYTESCLF), A(SUM, "@offset")]
DEFAULT, DIRECT, DIRECT_NO_PEEL = (0, 0), (-1, 0), (-1, -1)  # (OPT_GROUP_LDS_WORDS, OPT_GROUP_PEEL)
REGIMES = (DEFAULT, DIRECT, DIRECT_NO_PEEL)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _new_parser(fmt="combined"):
    """every path of the format and the request's query wildcard"""
    return lpa.HttpdLoglineParser(fmt, [f for f in lpa.get_possible_paths(fmt) if not f.endswith("*")] + [wc.QWILD])


@functools.lru_cache(None)
def _parser(fmt="combined"):
    """one handle per LogFormat for the tests that parse their own batch (a batch lives until the handle's next)"""
    return _new_parser(fmt)


def _option(r, option, value):
    assert lpa.lib().lp_set_option(r._p._h, option, value) == lpa.LP_OK, (option, value)


class Batch:
    """a parsed batch, its host copy and the host copy's decoded table columns (built once per column)"""

    def __init__(self, lines_status, parser=None):
        lines = [l for l, _ in lines_status]
        self.r = (parser or _parser()).parse_batch(rsc.join_lf(lines))
        assert self.r.n_lines == len(lines)
        assert self.r.status.tolist() == [s for _, s in lines_status]
        self.buf, self.res = self.r.copy_to_host()
        self.table = {}

    def need(self, keys, aggs):
        cols = {(k[0], k[1]) for k in keys} | {(a.path, int) for a in aggs if a.path}
        cols = sorted((c for c in cols if c not in self.table), key=lambda c: c[0])
        for typ in (str, int):  # (one table per kind: a path may be taken as both)
            part = [c for c in cols if c[1] is typ]
            if part:
                self.table.update(wc.decoded(self.r.table_from(self.res, part, threads=4, decode=False), part))

    def check(self, keys, aggs, first=0, count=None, rows=None, regimes=(DEFAULT, DIRECT)):
        """group_device (in each regime) == reference(the host copy's table) == group_from; returns the reference"""
        r = self.r
        self.need(keys, aggs)
        if rows is None:
            count = r.n_lines - first if count is None else count
            lines, dev_rows, kw = range(first, first + count), None, dict(first=first, count=count)
        else:
            import torch
            lines, kw = [int(x) for x in rows], {}
            dev_rows = torch.tensor(np.asarray(rows, dtype=np.int64), device="cuda:%d" % r._p.device)
        want = gc.reference(self.table, list(keys), list(aggs), lines)

        def same(got, what):
            assert got["n_groups"] == len(want[0]), (what, got["n_groups"], len(want[0]))
            assert _np(got["rep"]).tobytes() == want[0].tobytes(), (what, "rep", _np(got["rep"])[:8], want[0][:8])
            assert _np(got["group_of"]).tobytes() == want[1].tobytes(), (what, "group_of")
            assert len(got["aggs"]) == len(aggs)
            for a, (v, ok), (wv, wok) in zip(aggs, got["aggs"], want[2]):
                assert _np(ok).tobytes() == wok.tobytes(), (what, a, "valid", _np(ok)[:8], wok[:8])
                assert _np(v).tobytes() == wv.tobytes(), (what, a, "value", _np(v)[:8], wv[:8])

        try:
            for lds, peel in regimes:
                _option(r, lpa.OPT_GROUP_LDS_WORDS, lds)
                _option(r, lpa.OPT_GROUP_PEEL, peel)
                got = r.group_device(keys, aggs, rows=dev_rows, **kw)
                assert got["rep"].is_cuda and str(got["rep"].dtype) == "torch.int64"
                assert str(got["group_of"].dtype) == "torch.int32"
                same(got, ("device", lds, peel))
        finally:
            _option(r, lpa.OPT_GROUP_LDS_WORDS, 0)
            _option(r, lpa.OPT_GROUP_PEEL, 0)
        host = r.group_from(self.res, keys, aggs, rows=None if rows is None else np.asarray(rows, dtype=np.int64),
                            threads=3, decode=False, **kw)
        same(host, "host")
        return want


@functools.lru_cache(None)
def _mixed():
    """the batch several tests share, on a handle of its own: 700 lines of all three statuses"""
    return Batch(gc.mixed(700), parser=_new_parser())


@functools.lru_cache(None)
def _edges():
    return Batch(gc.edges(), parser=_new_parser())


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("n", (1, 63, 64, 65, 255, 256, 257, 4100))
def test_counts_gpu(n):
    """around a wave and a block, and several blocks flushing into the same groups"""
    b = Batch(gc.mixed(n))
    want = b.check([(STATUS, str)], FULL, regimes=REGIMES)
    assert len(want[0]) == len({None if s else gc.STATUSES[k * 3 % 8] for k, (_, s) in enumerate(gc.mixed(n))})
    b.check([(PATH, str), (METHOD, str)], BASIC)


def test_window_mid_batch_gpu():
    b = _mixed()
    for first, count in ((130, 333), (1, 64), (63, 2), (257, 443), (699, 1), (5, 0)):
        want = b.check([(METHOD, str)], FULL, first=first, count=count)
        assert count == 0 or want[0][0] == first  # the first group's first row is the window's
    assert b.check([(METHOD, str)], BASIC, first=5, count=0)[0].size == 0


def test_one_group_and_every_row_its_own_gpu():
    one = Batch(gc.same(300))
    want = one.check([(PATH, str)], FULL, regimes=REGIMES)
    assert want[0].tolist() == [0] and want[2][0][0].tolist() == [300]
    assert one.check([], FULL, regimes=REGIMES)[0].tolist() == [0]  # no keys: one group of every row
    each = Batch(gc.distinct(700))
    want = each.check([(PATH, str)], BASIC, regimes=REGIMES)
    assert want[0].tolist() == list(range(700)) and want[1].tolist() == list(range(700))
    assert each.check([("@line", str)], [A(ROWS), A(MAX, "@lineno")])[0].size == 700  # long key values


def test_hot_key_gpu():
    """one key on about 90 % of the rows between singletons: the wave peel's case, with every number of rounds"""
    b = Batch(gc.hot(4100))
    regimes = REGIMES + ((-1, 1), (-1, 4), (64, 0))
    want = b.check([(PATH, str)], FULL, regimes=regimes)
    assert len(want[0]) == 411 and want[2][0][0][1] == 4100 - 410
    b.check([(STATUS, str), (PATH, str)], BASIC, regimes=regimes)


def test_lds_budget_boundary_gpu():
    """the accumulator need at budget - 1, budget and budget + 1: both regimes on either side of the threshold"""
    b = _mixed()
    keys = [(PATH, str)]
    groups = len(b.check(keys, BASIC)[0])
    need = groups * gc.words(BASIC)
    assert groups == 38 and need == 114  # 37 paths and the null of the BAD / FALLBACK lines; three words each
    b.check(keys, BASIC, regimes=[(need + 1, 0), (need, 0), (need - 1, 0), (need - 1, -1), (1, 0), (8192, 0)])
    L, h = lpa.lib(), b.r._p._h
    assert L.lp_set_option(h, lpa.OPT_GROUP_LDS_WORDS, 8193) == lpa.LP_E_INVALID
    assert L.lp_set_option(h, lpa.OPT_GROUP_LDS_WORDS, -2) == lpa.LP_E_INVALID
    assert L.lp_set_option(h, lpa.OPT_GROUP_PEEL, 5) == lpa.LP_E_INVALID


def test_narrow_hash_gpu():
    """1 and 2 hash bits: distinct key tuples meet in the probe and in the full compare; the result stays"""
    b = _mixed()
    L, h = lpa.lib(), b.r._p._h
    try:
        for bits in (1, 2):
            assert L.lp_set_option(h, lpa.OPT_DICT_HASH_BITS, bits) == lpa.LP_OK
            b.check([(PATH, str)], FULL)
            b.check([(METHOD, str), (BYTES, int)], BASIC)
            b.check([("@lineno", int)], BASIC, first=100, count=300)  # every row its own group, all colliding
    finally:
        L.lp_set_option(h, lpa.OPT_DICT_HASH_BITS, 0)


def _raw(b, keys, aggs, cap, device):
    """one lp_result_group call with room for cap groups: (code, n_groups, rep, [(value, valid)])"""
    import torch
    r = b.r
    karr, aarr = lpa._group_args(keys, aggs)
    dev = "cuda:%d" % r._p.device
    mk = (lambda dt: torch.full((cap + 1,), 77, dtype=dt, device=dev)) if device else \
        (lambda dt: np.full(cap + 1, 77, dtype={torch.int64: np.int64, torch.uint8: np.uint8}[dt]))
    ptr = (lambda t: t.data_ptr()) if device else (lambda a: a.ctypes.data)
    rep, bufs = mk(torch.int64), [(mk(torch.int64), mk(torch.uint8)) for _ in aggs]
    for j, (v, ok) in enumerate(bufs):
        aarr[j].value, aarr[j].valid = ptr(v), ptr(ok)
    out = lpa.LpGroupOut()
    out.rep, out.groups_cap, out.n_groups = ptr(rep), cap, -1
    res = r._view() if device else b.res
    rc = lpa.lib().lp_result_group(r._p._h, ctypes.byref(res), 0, r.n_lines, karr, len(keys), aarr, len(aggs),
                                   ctypes.byref(out), 2)
    return rc, out.n_groups, _np(rep), [(_np(v), _np(ok)) for v, ok in bufs]


@pytest.mark.parametrize("device", (True, False), ids=("device", "host"))
def test_groups_cap_gpu(device):
    """one short: LP_E_NOMEM, the exact n_groups, nothing written; exact: filled, nothing past the capacity"""
    b = _mixed()
    want = b.check([(METHOD, str)], BASIC)
    n = len(want[0])
    assert n == 5
    rc, got_n, rep, aggs = _raw(b, [(METHOD, str)], BASIC, n - 1, device)
    assert (rc, got_n) == (lpa.LP_E_NOMEM, n)
    assert (rep == 77).all() and all((v == 77).all() and (ok == 77).all() for v, ok in aggs)
    rc, got_n, rep, aggs = _raw(b, [(METHOD, str)], BASIC, n, device)
    assert (rc, got_n) == (lpa.LP_OK, n) and rep[:n].tolist() == want[0].tolist() and rep[n] == 77
    for (v, ok), (wv, wok) in zip(aggs, want[2]):
        assert v[:n].tolist() == wv.tolist() and ok[:n].tolist() == wok.tolist() and v[n] == 77 and ok[n] == 77


# -------------------------------------------------------------------- 2. keys
KEYS = {"status-str": [(STATUS, str)], "method": [(METHOD, str)], "path": [(PATH, str)], "query-param": [(QP, str)],
        "date": [(DATE, str)], "bytes-clf2num": [(BYTES, int)], "bytesclf-long": [(BYTESCLF, int)],
        "bytesclf-str": [(BYTESCLF, str)], "epoch-str": [(EPOCH, str)],
        "@status": [("@status", int)], "@line": [("@line", str)],
        "two": [(METHOD, str), (BYTESCLF, int)], "four": [(METHOD, str), (STATUS, str), (DATE, str), (QP, str)]}


@pytest.mark.parametrize("name", sorted(KEYS))
def test_keys_gpu(name):
    """a token as STRING and as LONG, a first-line part, a URI part from the arena, a mostly-null query parameter,
    a formatted date, a converter, a long taken as STRING, the pseudo-columns over all statuses, composites"""
    want = _mixed().check(KEYS[name], FULL)
    assert len(want[0]) > 1
    _edges().check(KEYS[name], BASIC, regimes=REGIMES)


def test_status_as_long_follows_the_table_gpu():
    """STRING:request.status.last casts to STRING only (lp_casts): as a LONG key it is refused exactly as the
    table refuses the LONG column, before any launch; the status as a number is a LONG key through "@status"-like
    pseudo-columns or a path whose casts hold LONG"""
    b = _mixed()
    assert b.r._p.get_casts(STATUS) & lpa.CAST_LONG == 0
    with pytest.raises(ValueError):
        b.r.table_device([(STATUS, int)])
    with pytest.raises(ValueError):
        b.r.group_device([(STATUS, int)], BASIC)
    with pytest.raises(ValueError):
        b.r.group_from(b.res, [(STATUS, int)], BASIC)
    with pytest.raises(ValueError):
        b.r.group_device([(STATUS, str)], [A(SUM, STATUS)])  # a measure is LONG


def test_key_value_edges_gpu():
    b = _edges()
    # %b "007", "7", "00", "0": as LONG 7 and 0, as STRING four values; "-" and 9223372036854775808: null as LONG
    as_long = b.check([(BYTESCLF, int)], BASIC, regimes=REGIMES)
    assert sorted(x for x in {b.table[(BYTESCLF, int)][i] for i in as_long[0]} if x is not None) == [0, 5, 7, gc.I64_MAX]
    as_str = b.check([(BYTESCLF, str)], BASIC, regimes=REGIMES)
    assert {b.table[(BYTESCLF, str)][i] for i in as_str[0]} == {b"007", b"7", b"00", b"0", b"5", None, b"9223372036854775807",
                                                                b"9223372036854775808"}
    # BYTES through CLF2NUM: "-", "0" and "00" are one group
    clf = b.check([(BYTES, int)], BASIC)
    zero = [g for g, i in enumerate(clf[0]) if b.table[(BYTES, int)][i] == 0]
    assert len(zero) == 1 and clf[2][0][0][zero[0]] == 3 * 5
    # a composite in which only the last key differs
    only_last = Batch(gc.same(300))
    assert len(only_last.check([(METHOD, str), (STATUS, str), (PATH, str), (BYTES, int)], BASIC, regimes=REGIMES)[0]) == 7


# ---------------------------------------------------------------- 3. measures
def test_measures_gpu():
    """BYTES, @offset, the epoch of lines before 1970 (a negative minimum), a sum that wraps, a %b that is no long,
    a group whose measure is null on every row: eight aggregates over four distinct measures"""
    b = _edges()
    aggs = [A(SUM, BYTESCLF), A(MIN, EPOCH), A(MAX, EPOCH), A(CNT, BYTESCLF), A(SUM, "@offset"), A(ROWS), A(SUM, BYTES),
            A(MIN, BYTESCLF)]
    assert gc.words(aggs) == 1 + 4 + 6
    want = b.check([(PATH, str)], aggs, regimes=REGIMES)
    paths = [b.table[(PATH, str)][i] for i in want[0]]
    assert paths == [b"/w", b"/z", b"/n"]
    w, z, n = 0, 1, 2
    total = 3 * (2 * gc.I64_MAX + 5)
    assert want[2][0][0][w] == (total + (1 << 63)) % (1 << 64) - (1 << 63) and want[2][0][0][w] != total  # wrapped
    assert want[2][1][0][z] < 0 and want[2][1][1][z] == 1  # 1968: before the epoch
    assert want[2][0][1][n] == 0 and want[2][7][1][n] == 0 and want[2][3][0][n] == 0  # null on every row: valid 0, COUNT 0
    assert want[2][3][1][n] == 1 and want[2][5][0][n] == 9  # ... COUNT itself is valid; the rows are counted
    _mixed().check([(STATUS, str)], aggs)


# --------------------------------------------------------------- 4. row lists
def test_row_lists_gpu():
    b = _mixed()
    r = b.r
    sel = r.select_where_device([lpa.Where(STATUS, lpa.WHERE_PREFIX, "5")])  # the 5xx lines
    assert sel.numel() > 50
    got = r.group_device([(STATUS, str)], BASIC, rows=sel)  # the select's output goes straight in
    rows = _np(sel)
    want = b.check([(STATUS, str)], BASIC, rows=rows, regimes=REGIMES)
    assert _np(got["rep"]).tobytes() == want[0].tobytes() and got["n_groups"] == 2
    # repeated and reversed: the order follows k, rep is the line
    back = np.concatenate([rows[::-1], rows[:40], rows[::-1][:7]])
    want = b.check([(PATH, str)], FULL, rows=back, regimes=REGIMES)
    assert want[0][0] == rows[-1]
    # BAD and FALLBACK lines in the list: null in every real column, their pseudo-columns valid
    every = _np(r.select_device(7))[::-1].copy()
    want = b.check([(METHOD, str), ("@status", int)], FULL, rows=every)
    assert {b.table[("@status", int)][i] for i in want[0]} == {0, 1, 2}
    b.check([(METHOD, str)], BASIC, rows=np.zeros(0, dtype=np.int64))
    b.check([(METHOD, str)], BASIC, rows=np.array([5, 5, 5], dtype=np.int64))


def test_two_logformats_gpu():
    """combined and common lines interleaved: the user agent is null on a common line"""
    n = 300
    ls = [(wc.common_line(k), 0) if k % 3 == 1 else (wc.ok_line(k), 0) for k in range(n)]
    b = Batch(ls, parser=_parser("combined\ncommon"))
    want = b.check([(wc.UA, str)], BASIC, regimes=REGIMES)
    null = [g for g, i in enumerate(want[0]) if b.table[(wc.UA, str)][i] is None]
    assert len(null) == 1 and want[2][0][0][null[0]] == n // 3
    b.check([(STATUS, str), (wc.REFERER, str)], FULL)


# ------------------------------------------------------- 5. the API's contract
def test_decode_timing_and_empty_gpu():
    b = _mixed()
    r = b.r
    t = (ctypes.c_float * 23)(*([-1.0] * 23))
    host = r.group_from(b.res, [(METHOD, str), (BYTES, int)], BASIC)
    assert host["keys"][METHOD][0] == [b.table[(METHOD, str)][i].decode() if b.table[(METHOD, str)][i] is not None else None
                                       for i in host["rep"]]
    assert host["keys"][BYTES][0].tolist() == [b.table[(BYTES, int)][i] or 0 for i in host["rep"]]
    r.group_device([(METHOD, str)], BASIC)
    timing = r.group_timing()
    assert set(timing) == {"insert", "index", "aggregate"} and all(v > 0 for v in timing.values())
    assert lpa.lib().lp_last_timing(r._p._h, t, 20) == 20 and t[20] == -1.0  # a caller of 20 sees what it always saw
    assert lpa.lib().lp_last_timing(r._p._h, t, 23) == 23 and t[20] == pytest.approx(timing["insert"])
    got = r.group_device([(METHOD, str)], BASIC, first=3, count=0)  # an empty call: no launch, the timing stays
    assert got["n_groups"] == 0 and got["rep"].numel() == 0 and r.group_timing() == timing
    got = r.group_device([(METHOD, str)], BASIC, groups_cap=64)  # room allotted at once: one call
    assert got["n_groups"] == 5
    assert r.table_device([(METHOD, str)], first=0, count=1) is not None  # the next table call is unharmed


def test_host_checks_gpu():
    """what the host refuses before any launch, with its code; the row indices on the host path"""
    b = _mixed()
    r, L = b.r, lpa.lib()
    with pytest.raises(ValueError):
        r.group_from(b.res, [(METHOD, str)], BASIC, rows=np.array([0, r.n_lines], dtype=np.int64))
    with pytest.raises(ValueError):
        r.group_from(b.res, [(METHOD, str)], BASIC, rows=np.array([-1], dtype=np.int64))
    with pytest.raises(ValueError):
        r.group_from(b.res, [(METHOD, str)], BASIC, first=1, count=r.n_lines)
    with pytest.raises(lpa.MissingDissectorsException):
        r.group_device([("STRING:no.such.path", str)], BASIC)
    with pytest.raises(lpa.MissingDissectorsException):
        r.group_device([(METHOD, str)], [A(SUM, "BYTES:no.such.path")])
    with pytest.raises(ValueError):
        r.group_device([("@line", int)], BASIC)  # the wrong kind for a pseudo-column
    res, out = r._view(), lpa.LpGroupOut()
    karr, aarr = lpa._group_args([(METHOD, str)], [A(ROWS)])
    call = lambda nk, na, k=karr, a=aarr: L.lp_result_group(r._p._h, ctypes.byref(res), 0, r.n_lines, k, nk, a, na,  # noqa: E731
                                                            ctypes.byref(out), 1)
    assert call(5, 1) == lpa.LP_E_INVALID and call(-1, 1) == lpa.LP_E_INVALID and call(1, 9) == lpa.LP_E_INVALID
    assert call(1, 1, None) == lpa.LP_E_INVALID and call(1, 1, karr, None) == lpa.LP_E_INVALID
    aarr[0].op = 7
    assert call(1, 1) == lpa.LP_E_INVALID  # an unknown op
    aarr[0].op, aarr[0].path = ROWS, b"BYTES:response.body.bytes"
    assert call(1, 1) == lpa.LP_E_INVALID  # a path on COUNT_ROWS
    aarr[0].op, aarr[0].path = SUM, None
    assert call(1, 1) == lpa.LP_E_INVALID  # no path where one is needed
    karr[0].kind = lpa.CAST_DOUBLE
    aarr[0].op = ROWS
    assert call(1, 1) == lpa.LP_E_INVALID  # a key is LONG or STRING
    karr[0].kind = lpa.CAST_STRING
    assert call(1, 1) == lpa.LP_E_NOMEM and out.n_groups == 5  # (no room given: the count)
    assert L.lp_result_group(r._p._h, ctypes.byref(res), 0, 1 << 31, karr, 1, aarr, 1, ctypes.byref(out), 1) == lpa.LP_E_INVALID
    out.groups_cap = -1
    assert call(1, 1) == lpa.LP_E_INVALID
