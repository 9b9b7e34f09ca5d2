"""The C ABI contract of the typed-table families (lp_result_table / _dict /
_map and their _rows forms, lp_result_select): which code a malformed call
returns, and which wins when two faults apply -- on the device view and on a
host copy.  EXPECTED is a literal table: include/logparser_amd.h where it
states the code, otherwise the behaviour recorded from the commit before the
host layer's checks were gathered into shared helpers (profiles/table_api/
contract_parent.log).  The second half pins the host worker split: any thread
count gives the arrays of one thread, and those of the device.

One batch of 130 'combined' lines (three waves, the last partial), so windows
and row lists cross a 64-line boundary and reach the last line.

A row list with an index outside the batch is given on the host copy only: as
in test_row_select_gpu.py, the device-side bound check is not exercised on a
shared machine."""
import ctypes

import numpy as np
import pytest

import dict_corpus as dc
import logparser_amd as lpa

pytestmark = pytest.mark.gpu

N = 130
MAX_TABLE_COLS = 32  # csrc/lp_table.h
OK, INV, MISS, UNS, NOMEM, STATE = (lpa.LP_OK, lpa.LP_E_INVALID, lpa.LP_E_MISSING, lpa.LP_E_UNSUPPORTED,
                                    lpa.LP_E_NOMEM, lpa.LP_E_STATE)
S, L_, D = lpa.CAST_STRING, lpa.CAST_LONG, lpa.CAST_DOUBLE
EPOCH = "TIME.EPOCH:request.receive.time.epoch"
REF = "STRING:request.referer.query.*"
# A remapped delivery itself: only the host replay derives it.  (The issue's DOUBLE column over a
# host-only source cannot be built: a retyped target's casts are STRING only, and the one DOUBLE
# cast the formats have, a SECOND_MILLIS list item, is converted on the device.)
NUM = "NUM:request.firstline.uri.query.a"
UNTOUCHED = 0x5A5A5A5A5A5A5A5A  # a *_len the call did not set


def _ua(k):
    return b"agent-%d" % (k % 11)


def _ref(k):
    return b"http://r.example/p?r=%d" % k


LINES = [dc.line(k, ua=_ua(k), ref=_ref(k)) for k in range(N)]
# what the size protocol must report, from the corpus itself
NEED_UA = sum(len(_ua(k)) for k in range(N))
NEED_PATH = sum(len(b"/p%d" % (k % 7)) for k in range(N))
NEED_REQ = (2 * N, 2 * N, sum(len(b"%d" % (k % 5)) for k in range(N)))  # ?e=&a=K: entries, key bytes, value bytes
NEED_REF = (N, N, sum(len(b"%d" % k) for k in range(N)))                # ?r=K
DICT_UA = (11, sum(len(_ua(k)) for k in range(11)))
DICT_PATH = (7, sum(len(b"/p%d" % k) for k in range(7)))


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class Env:
    """one view of the module's batch: its handle, lp_result and how to make memory of its side"""

    def __init__(self, r, res, on_host, keep=None):
        self.r, self.h, self.res, self.on_host, self.keep = r, r._p._h, res, on_host, keep

    def mk(self, nbytes):
        if self.on_host:
            return np.full(nbytes + 8, 0x5A, dtype=np.uint8)
        import torch
        return torch.full((nbytes + 8,), 0x5A, dtype=torch.uint8, device="cuda")

    def ptr(self, a):
        return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()

    def rows(self, values):
        a = np.ascontiguousarray(values, dtype=np.int64)
        if self.on_host:
            return a
        import torch
        return torch.from_numpy(a).cuda()


def _view(r):
    v = lpa.LpResult()
    assert lpa.lib().lp_result_view(r._p._h, ctypes.byref(v)) == OK
    return v


@pytest.fixture(scope="module")
def envs():
    fields = [f for f in lpa.get_possible_paths(dc.FMT) if not f.endswith("*")] + [dc.REQ, REF]
    data = dc.join_lf(LINES)
    p = lpa.HttpdLoglineParser(dc.FMT, fields)
    r = p.parse_batch(data)
    assert r.n_lines == N and r.status.tolist() == [lpa.LINE_OK] * N
    hbuf, hres = r.copy_to_host()
    # a view that a later batch of its handle made stale
    p2 = lpa.HttpdLoglineParser(dc.FMT, fields)
    stale = _view(p2.parse_batch(data))
    r2 = p2.parse_batch(data)
    # a handle with a path whose values only the host replay derives
    q = lpa.HttpdLoglineParser(dc.FMT, [NUM])
    q.add_type_remapping("request.firstline.uri.query.a", "NUM", lpa.STRING_OR_LONG_OR_DOUBLE)
    rq = q.parse_batch(data)
    assert rq.n_lines == N and q.get_casts(NUM) == S
    qbuf, qres = rq.copy_to_host()
    return {"device": Env(r, _view(r), False), "host": Env(r, hres, True, hbuf),
            "stale": Env(r2, stale, False), "num_device": Env(rq, _view(rq), False), "num_host": Env(rq, qres, True, qbuf)}


# ---------------------------------------------------------------- raw callers
def _table_cols(e, specs, n=N, caps=None):
    cols = (lpa.LpTableCol * max(1, len(specs)))()
    keep = []
    for k, (path, kind) in enumerate(specs):
        c = cols[k]
        c.path = None if path is None else path.encode()
        c.kind = kind
        cap = 4096 if caps is None else caps[k]
        b = [e.mk(n), e.mk(8 * (n + 1)), e.mk(8 * n), e.mk(cap)]
        c.valid, c.i64, c.f64, c.chars = (e.ptr(x) for x in b)
        c.chars_cap, c.chars_len = cap, UNTOUCHED
        keep.append(b)
    return cols, keep


def _dict_cols(e, paths, n=N, caps=None):
    cols = (lpa.LpTableDictCol * max(1, len(paths)))()
    keep = []
    for k, path in enumerate(paths):
        c = cols[k]
        c.path = None if path is None else path.encode()
        dcap, ccap = (64, 4096) if caps is None else caps[k]
        b = [e.mk(n), e.mk(4 * n), e.mk(8 * (dcap + 1)), e.mk(ccap)]
        c.valid, c.index, c.dict_off, c.dict_chars = (e.ptr(x) for x in b)
        c.dict_cap, c.dict_chars_cap, c.dict_len, c.dict_chars_len = dcap, ccap, -77, UNTOUCHED
        keep.append(b)
    return cols, keep


def _map_cols(e, paths, n=N, caps=None):
    cols = (lpa.LpTableMapCol * max(1, len(paths)))()
    keep = []
    for k, path in enumerate(paths):
        c = cols[k]
        c.path = None if path is None else path.encode()
        ecap, kcap, vcap = (512, 4096, 4096) if caps is None else caps[k]
        b = [e.mk(n), e.mk(8 * (n + 1)), e.mk(8 * (ecap + 1)), e.mk(8 * (ecap + 1)), e.mk(kcap), e.mk(vcap)]
        c.valid, c.entry_off, c.key_off, c.val_off, c.key_chars, c.val_chars = (e.ptr(x) for x in b)
        c.entries_cap, c.key_chars_cap, c.val_chars_cap = ecap, kcap, vcap
        c.entries_len = c.key_chars_len = c.val_chars_len = UNTOUCHED
        keep.append(b)
    return cols, keep


_FN = {"table": ("lp_result_table", "lp_result_table_rows"), "table_dict": ("lp_result_table_dict", "lp_result_table_dict_rows"),
       "table_map": ("lp_result_table_map", "lp_result_table_map_rows")}
_COLS = {"table": _table_cols, "table_dict": _dict_cols, "table_map": _map_cols}
_NULL = object()
HOST_ROWS = np.array([3, 0, 129], dtype=np.int64)


def _call(fam, e, cols, n_cols, first=0, count=N, rows=None, n_rows=None, threads=2):
    """rows: None (the window form), _NULL (the rows form with a null list) or an array / tensor / raw pointer"""
    Lb = lpa.lib()
    if rows is None:
        return getattr(Lb, _FN[fam][0])(e.h, ctypes.byref(e.res), first, count, cols, n_cols, threads)
    rp = None if rows is _NULL else rows if isinstance(rows, int) else e.ptr(rows)
    n_rows = n_rows if n_rows is not None else 0 if rows is _NULL or isinstance(rows, int) else len(rows)
    return getattr(Lb, _FN[fam][1])(e.h, ctypes.byref(e.res), rp, n_rows, cols, n_cols, threads)


def _simple(fam, e, specs, **kw):
    cols, keep = _COLS[fam](e, specs)
    return _call(fam, e, cols, len(specs), **kw)


def _capped(fam, e, specs, caps, mem=None):
    """a call whose columns have the capacities caps (their arrays made by mem, default the view's own side)"""
    cols, keep = _COLS[fam](mem or e, specs, caps=caps)
    return _call(fam, e, cols, len(specs))


def _select(e, first=0, count=N, mask=lpa.SEL_OK, cap=N, rows_len=True, host_rows=False):
    n = ctypes.c_uint64(UNTOUCHED)
    buf = np.full(8 * cap + 8, 0x5A, dtype=np.uint8) if host_rows else e.mk(8 * cap)
    rc = lpa.lib().lp_result_select(e.h, ctypes.byref(e.res), first, count, mask, e.ptr(buf), cap,
                                    ctypes.byref(n) if rows_len else None)
    return rc, int(n.value), buf


# ------------------------------------------------------------- the fault cases
# per family: {case: (what a valid column list looks like is in GOOD) a function of (envs, view) -> code}
GOOD = {"table": [(dc.UA, S), (EPOCH, L_)], "table_dict": [dc.UA, dc.PATH], "table_map": [dc.REQ, REF]}
UNKNOWN = {"table": [("STRING:request.nothing", S)], "table_dict": ["STRING:request.nothing"],
           "table_map": ["STRING:request.nothing.*"]}


def _null_array(fam, e, field, kind=S):
    specs = [(dc.UA if kind == S else EPOCH, kind)] if fam == "table" else GOOD[fam][:1]
    cols, keep = _COLS[fam](e, specs)
    setattr(cols[0], field, None)
    return _call(fam, e, cols, 1)


def _many(fam, e):
    specs = {"table": [(EPOCH, L_)], "table_dict": [dc.UA], "table_map": [dc.REQ]}[fam] * (MAX_TABLE_COLS + 1)
    return _simple(fam, e, specs)


def _zero_cols(fam, e):
    cols, keep = _COLS[fam](e, GOOD[fam])
    return _call(fam, e, cols, 0)


def _common_cases(fam):
    """the faults every column family has: case -> f(envs, view name) -> code"""
    good = GOOD[fam]
    c = {
        "null cols": lambda E, v: _call(fam, E[v], None, 1),
        "n_cols 0": lambda E, v: _zero_cols(fam, E[v]),
        "n_cols 33": lambda E, v: _many(fam, E[v]),
        "null path": lambda E, v: _simple(fam, E[v], [(None, S)] if fam == "table" else [None]),
        "null valid": lambda E, v: _null_array(fam, E[v], "valid"),
        "unknown path": lambda E, v: _simple(fam, E[v], UNKNOWN[fam]),
        "first -1": lambda E, v: _simple(fam, E[v], good, first=-1, count=1),
        "count -1": lambda E, v: _simple(fam, E[v], good, first=0, count=-1),
        "window one past the batch": lambda E, v: _simple(fam, E[v], good, first=1, count=N),
        "n_rows -1": lambda E, v: _simple(fam, E[v], good, rows=E[v].rows([1, 2]), n_rows=-1),
        "n_rows 2, null rows": lambda E, v: _simple(fam, E[v], good, rows=_NULL, n_rows=2),
        "n_rows -1, rows not of the view's side": lambda E, v: _simple(
            fam, E[v], good, rows=E["host" if v == "device" else "device"].rows([1, 2]), n_rows=-1),
    }
    return c


def _view_cases(fam):
    """faults of one view only: case -> (view, f(envs) -> code)"""
    good = GOOD[fam]
    return {
        "stale view": ("device", lambda E: _simple(fam, E["stale"], good)),
        "unknown path and stale view": ("device", lambda E: _simple(fam, E["stale"], UNKNOWN[fam])),
        "bad window and stale view": ("device", lambda E: _simple(fam, E["stale"], good, first=1, count=N)),
        "host pointer as rows": ("device", lambda E: _simple(fam, E["device"], good, rows=HOST_ROWS.ctypes.data,
                                                            n_rows=3)),
        "rows with -1": ("host", lambda E: _simple(fam, E["host"], good, rows=E["host"].rows([3, -1, 5]))),
        "rows with n_lines": ("host", lambda E: _simple(fam, E["host"], good, rows=E["host"].rows([3, N, 5]))),
    }


CASES = {fam: _common_cases(fam) for fam in _FN}
VIEW_CASES = {fam: _view_cases(fam) for fam in _FN}
CASES["table"].update({
    "null i64 of a STRING column": lambda E, v: _null_array("table", E[v], "i64", S),
    "null i64 of a LONG column": lambda E, v: _null_array("table", E[v], "i64", L_),
    "null f64 of a DOUBLE column": lambda E, v: _null_array("table", E[v], "f64", D),
    "kind 0": lambda E, v: _simple("table", E[v], [(dc.UA, 0)]),
    "kind 3": lambda E, v: _simple("table", E[v], [(dc.UA, 3)]),
    "kind 8": lambda E, v: _simple("table", E[v], [(dc.UA, 8)]),
    "unknown pseudo-column": lambda E, v: _simple("table", E[v], [("@nothing", S)]),
    "casts exclude the kind": lambda E, v: _simple("table", E[v], [(dc.UA, L_)]),
    "@line as LONG": lambda E, v: _simple("table", E[v], [("@line", L_)]),
    "@offset as STRING": lambda E, v: _simple("table", E[v], [("@offset", S)]),
    "a host-only source": lambda E, v: _simple("table", E["num_" + v], [(NUM, S)]),
    "a host-only source as DOUBLE": lambda E, v: _simple("table", E["num_" + v], [(NUM, D)]),
    "casts exclude the kind and a short capacity": lambda E, v: _capped(
        "table", E[v], [(dc.UA, S), (dc.UA, L_)], [0, 0]),
})
CASES["table_dict"].update({
    "null index": lambda E, v: _null_array("table_dict", E[v], "index"),
    "null dict_off": lambda E, v: _null_array("table_dict", E[v], "dict_off"),
    "dict_cap -1": lambda E, v: _capped("table_dict", E[v], [dc.UA], [(-1, 64)]),
    "unknown pseudo-column": lambda E, v: _simple("table_dict", E[v], ["@nothing"]),
    "@offset": lambda E, v: _simple("table_dict", E[v], ["@offset"]),
    "@status and a short capacity": lambda E, v: _capped(
        "table_dict", E[v], [dc.UA, "@status"], [(0, 0), (0, 0)]),
    "count 2^31 with null arrays": lambda E, v: lpa.lib().lp_result_table_dict(
        E[v].h, ctypes.byref(E[v].res), 0, 1 << 31, ctypes.byref(lpa.LpTableDictCol()), 1, 1),
    "n_rows 2^31 with null arrays": lambda E, v: lpa.lib().lp_result_table_dict_rows(
        E[v].h, ctypes.byref(E[v].res), E[v].ptr(E[v].rows([0])), 1 << 31, ctypes.byref(lpa.LpTableDictCol()), 1, 1),
})
CASES["table_map"].update({
    "null entry_off": lambda E, v: _null_array("table_map", E[v], "entry_off"),
    "null key_off": lambda E, v: _null_array("table_map", E[v], "key_off"),
    "null val_off": lambda E, v: _null_array("table_map", E[v], "val_off"),
    "path not ending .*": lambda E, v: _simple("table_map", E[v], [dc.UA]),
    "pseudo-column": lambda E, v: _simple("table_map", E[v], ["@line"]),
    "not a wildcard and a short capacity": lambda E, v: _capped(
        "table_map", E[v], [dc.REQ, dc.UA], [(0, 0, 0), (0, 0, 0)]),
})
VIEW_CASES["table_dict"]["host arrays"] = ("device", lambda E: _capped(
    "table_dict", E["device"], [dc.UA], None, mem=E["host"]))

# (family, case) -> (code on the device view, code on a host copy); None: the case does not apply there
EXPECTED = {
    ("table", "null cols"): (INV, INV),
    ("table", "n_cols 0"): (INV, INV),
    ("table", "n_cols 33"): (INV, OK),
    ("table", "null path"): (INV, INV),
    ("table", "null valid"): (INV, INV),
    ("table", "null i64 of a STRING column"): (INV, INV),
    ("table", "null i64 of a LONG column"): (INV, INV),
    ("table", "null f64 of a DOUBLE column"): (INV, INV),
    ("table", "kind 0"): (INV, INV),
    ("table", "kind 3"): (INV, INV),
    ("table", "kind 8"): (INV, INV),
    ("table", "unknown path"): (MISS, MISS),
    ("table", "unknown pseudo-column"): (MISS, MISS),
    ("table", "casts exclude the kind"): (INV, INV),
    ("table", "@line as LONG"): (INV, INV),
    ("table", "@offset as STRING"): (INV, INV),
    ("table", "a host-only source"): (UNS, OK),
    ("table", "a host-only source as DOUBLE"): (INV, INV),
    ("table", "first -1"): (INV, INV),
    ("table", "count -1"): (INV, INV),
    ("table", "window one past the batch"): (INV, INV),
    ("table", "n_rows -1"): (INV, INV),
    ("table", "n_rows 2, null rows"): (INV, INV),
    ("table", "n_rows -1, rows not of the view's side"): (INV, INV),
    ("table", "casts exclude the kind and a short capacity"): (INV, INV),
    ("table", "stale view"): (STATE, None),
    ("table", "unknown path and stale view"): (MISS, None),
    ("table", "bad window and stale view"): (STATE, None),
    ("table", "host pointer as rows"): (INV, None),
    ("table", "rows with -1"): (None, INV),
    ("table", "rows with n_lines"): (None, INV),
    ("table_dict", "null cols"): (INV, INV),
    ("table_dict", "n_cols 0"): (INV, INV),
    ("table_dict", "n_cols 33"): (INV, OK),
    ("table_dict", "null path"): (INV, INV),
    ("table_dict", "null valid"): (INV, INV),
    ("table_dict", "null index"): (INV, INV),
    ("table_dict", "null dict_off"): (INV, INV),
    ("table_dict", "dict_cap -1"): (INV, INV),
    ("table_dict", "unknown path"): (MISS, MISS),
    ("table_dict", "unknown pseudo-column"): (MISS, MISS),
    ("table_dict", "@offset"): (INV, INV),
    ("table_dict", "@status and a short capacity"): (INV, INV),
    ("table_dict", "count 2^31 with null arrays"): (INV, INV),
    ("table_dict", "n_rows 2^31 with null arrays"): (INV, INV),
    ("table_dict", "first -1"): (INV, INV),
    ("table_dict", "count -1"): (INV, INV),
    ("table_dict", "window one past the batch"): (INV, INV),
    ("table_dict", "n_rows -1"): (INV, INV),
    ("table_dict", "n_rows 2, null rows"): (INV, INV),
    ("table_dict", "n_rows -1, rows not of the view's side"): (INV, INV),
    ("table_dict", "stale view"): (STATE, None),
    ("table_dict", "unknown path and stale view"): (MISS, None),
    ("table_dict", "bad window and stale view"): (STATE, None),
    ("table_dict", "host pointer as rows"): (INV, None),
    ("table_dict", "host arrays"): (INV, None),
    ("table_dict", "rows with -1"): (None, INV),
    ("table_dict", "rows with n_lines"): (None, INV),
    ("table_map", "null cols"): (INV, INV),
    ("table_map", "n_cols 0"): (INV, INV),
    ("table_map", "n_cols 33"): (OK, OK),
    ("table_map", "null path"): (INV, INV),
    ("table_map", "null valid"): (INV, INV),
    ("table_map", "null entry_off"): (INV, INV),
    ("table_map", "null key_off"): (INV, INV),
    ("table_map", "null val_off"): (INV, INV),
    ("table_map", "path not ending .*"): (INV, INV),
    ("table_map", "pseudo-column"): (INV, INV),
    ("table_map", "not a wildcard and a short capacity"): (INV, INV),
    ("table_map", "unknown path"): (MISS, MISS),
    ("table_map", "first -1"): (INV, INV),
    ("table_map", "count -1"): (INV, INV),
    ("table_map", "window one past the batch"): (INV, INV),
    ("table_map", "n_rows -1"): (INV, INV),
    ("table_map", "n_rows 2, null rows"): (INV, INV),
    ("table_map", "n_rows -1, rows not of the view's side"): (INV, INV),
    ("table_map", "stale view"): (STATE, None),
    ("table_map", "unknown path and stale view"): (MISS, None),
    ("table_map", "bad window and stale view"): (STATE, None),
    ("table_map", "host pointer as rows"): (INV, None),
    ("table_map", "rows with -1"): (None, INV),
    ("table_map", "rows with n_lines"): (None, INV),
    ("select", "null rows_len"): (INV, INV),
    ("select", "unknown mask bit"): (INV, INV),
    ("select", "first -1"): (INV, INV),
    ("select", "count -1"): (INV, INV),
    ("select", "window one past the batch"): (INV, INV),
    ("select", "stale view"): (STATE, None),
    ("select", "unknown mask bit and stale view"): (INV, None),
    ("select", "bad window and stale view"): (STATE, None),
    ("select", "host pointer as rows"): (INV, None),
}
SELECT_CASES = {
    "null rows_len": lambda E, v: _select(E[v], rows_len=False)[0],
    "unknown mask bit": lambda E, v: _select(E[v], mask=lpa.SEL_OK | 8)[0],
    "first -1": lambda E, v: _select(E[v], first=-1, count=1)[0],
    "count -1": lambda E, v: _select(E[v], count=-1)[0],
    "window one past the batch": lambda E, v: _select(E[v], first=1, count=N)[0],
}
SELECT_VIEW_CASES = {
    "stale view": ("device", lambda E: _select(E["stale"])[0]),
    "unknown mask bit and stale view": ("device", lambda E: _select(E["stale"], mask=16)[0]),
    "bad window and stale view": ("device", lambda E: _select(E["stale"], first=1, count=N)[0]),
    "host pointer as rows": ("device", lambda E: _select(E["device"], host_rows=True)[0]),
}


@pytest.mark.parametrize("view", ["device", "host"])
@pytest.mark.parametrize("fam", ["table", "table_dict", "table_map", "select"])
def test_fault_codes_gpu(envs, fam, view):
    """every malformed call of the family on the view: the whole table is printed, then compared"""
    col = 0 if view == "device" else 1
    common = SELECT_CASES if fam == "select" else CASES[fam]
    single = SELECT_VIEW_CASES if fam == "select" else VIEW_CASES[fam]
    got = {case: f(envs, view) for case, f in common.items()}
    got.update({case: f(envs) for case, (v, f) in single.items() if v == view})
    want = {case: codes[col] for (f_, case), codes in EXPECTED.items() if f_ == fam and codes[col] is not None}
    for case in sorted(set(got) | set(want)):
        print("CONTRACT %s | %s | %s -> %s (expected %s)" % (fam, view, case, got.get(case), want.get(case)))
    assert got == want
    # the view still serves a well-formed call after all of them
    if fam == "select":
        rc, n, buf = _select(envs[view])
        assert (rc, n) == (OK, N) and _np(buf)[:8 * N].view(np.int64).tolist() == list(range(N))
    else:
        assert _simple(fam, envs[view], GOOD[fam]) == OK


# ------------------------------------------------------------ the size protocol
def _lens(fam, cols, n):
    if fam == "table":
        return [int(cols[k].chars_len) for k in range(n)]
    if fam == "table_dict":
        return [(int(cols[k].dict_len), int(cols[k].dict_chars_len)) for k in range(n)]
    return [(int(cols[k].entries_len), int(cols[k].key_chars_len), int(cols[k].val_chars_len)) for k in range(n)]


SIZED = {"table": ([(dc.UA, S), (dc.PATH, S)], [NEED_UA, NEED_PATH]),
         "table_dict": ([dc.UA, dc.PATH], [DICT_UA, DICT_PATH]),
         "table_map": ([dc.REQ, REF], [NEED_REQ, NEED_REF])}
# is the valid column after a column that was LP_E_NOMEM filled?  (family, view) -> as the parent did
LATER_FILLED = {("table", "device"): False, ("table", "host"): True, ("table_dict", "device"): True,
                ("table_dict", "host"): True, ("table_map", "device"): False, ("table_map", "host"): True}


def _short(need):
    return need - 1 if isinstance(need, int) else tuple(x - 1 for x in need)


def _payload(fam, keep_k):
    """the bytes of a column's last array (chars / dict_chars / val_chars) as the call left them"""
    return _np(keep_k[-1])


@pytest.mark.parametrize("view", ["device", "host"])
@pytest.mark.parametrize("fam", ["table", "table_dict", "table_map"])
def test_size_protocol_gpu(envs, fam, view):
    e = envs[view]
    specs, need = SIZED[fam]
    # every capacity one short: LP_E_NOMEM, and every length of every column reported
    cols, keep = _COLS[fam](e, specs, caps=[_short(x) for x in need])
    rc = _call(fam, e, cols, 2)
    print("CONTRACT %s | %s | every capacity one short -> %s lens %s (expected %s)" % (fam, view, rc, _lens(fam, cols, 2), need))
    assert rc == NOMEM and _lens(fam, cols, 2) == need
    # the exact-fit repeat
    cols, keep = _COLS[fam](e, specs, caps=need)
    rc = _call(fam, e, cols, 2)
    print("CONTRACT %s | %s | exact fit -> %s lens %s" % (fam, view, rc, _lens(fam, cols, 2)))
    assert rc == OK and _lens(fam, cols, 2) == need
    exact = [_payload(fam, k).copy() for k in keep]
    last = need[1] if isinstance(need[1], int) else need[1][-1]
    assert not (exact[1][:last] == 0x5A).all() and (exact[1][last:] == 0x5A).all()
    # a short column, then a valid one: its lengths are set all the same
    cols, keep = _COLS[fam](e, specs, caps=[_short(need[0]), need[1]])
    rc = _call(fam, e, cols, 2)
    filled = bool((_payload(fam, keep[1]) == exact[1]).all())
    untouched = bool((_payload(fam, keep[1]) == 0x5A).all())
    print("CONTRACT %s | %s | a short column, then a valid one -> %s lens %s later column filled %s untouched %s (expected %s)"
          % (fam, view, rc, _lens(fam, cols, 2), filled, untouched, LATER_FILLED[(fam, view)]))
    assert rc == NOMEM and _lens(fam, cols, 2) == need
    assert (filled, untouched) == (LATER_FILLED[(fam, view)], not LATER_FILLED[(fam, view)])


@pytest.mark.parametrize("view", ["device", "host"])
def test_select_size_protocol_gpu(envs, view):
    e = envs[view]
    rc, n, buf = _select(e, cap=N - 1)
    print("CONTRACT select | %s | capacity one short -> %s rows_len %s" % (view, rc, n))
    assert (rc, n) == (NOMEM, N) and (_np(buf) == 0x5A).all()  # nothing written
    rc, n, buf = _select(e, cap=N)
    assert (rc, n) == (OK, N) and _np(buf)[:8 * N].view(np.int64).tolist() == list(range(N))


# --------------------------------------------------------- the host worker split
COUNTS = (0, 1, 3, 130)
THREADS = (0, 1, 16, 64, 100)
FIRST = {0: 5, 1: N - 1, 3: 62, 130: 0}  # a window at the last line, one across a wave boundary
TCOLS = [(dc.UA, str), (EPOCH, int), ("@line", str), ("@lineno", int), (dc.PARAM_A, str)]


def _row_lists(count):
    return {"reversed": np.arange(N - 1, -1, -1, dtype=np.int64)[:count].copy(),
            "repeats": np.array([63 + k % 3 if k % 2 else N - 1 - k % 4 for k in range(count)], dtype=np.int64)}


def _flat(out):
    """every array of a table_* result, in a fixed order, as bytes"""
    parts = []

    def walk(x):
        if isinstance(x, dict):
            for k in sorted(x):
                walk(x[k])
        elif isinstance(x, (tuple, list)):
            for y in x:
                walk(y)
        else:
            a = _np(x)
            parts.append(a.astype(np.uint8).tobytes() if a.dtype == bool else a.tobytes())
    walk(out)
    return parts


@pytest.mark.parametrize("count", COUNTS)
def test_host_chunks_gpu(envs, count):
    """threads above count and a count threads does not divide leave empty trailing chunks"""
    import torch
    r, res = envs["host"].r, envs["host"].res
    selections = [("window", {"first": FIRST[count], "count": count}, {"first": FIRST[count], "count": count})]
    selections += [(name, {"rows": a}, {"rows": torch.from_numpy(a).cuda()}) for name, a in _row_lists(count).items()]
    for name, hkw, dkw in selections:
        dev = (_flat(r.table_device(TCOLS, **dkw)), _flat(r.table_dict_device([dc.UA, dc.PATH], **dkw)),
               _flat(r.table_map_device([dc.REQ, REF], decode=False, **dkw)))
        one = None
        for threads in (1,) + THREADS:
            got = (_flat(r.table_from(res, TCOLS, threads=threads, decode=False, **hkw)),
                   _flat(r.table_dict_from(res, [dc.UA, dc.PATH], threads=threads, **hkw)),
                   _flat(r.table_map_from(res, [dc.REQ, REF], threads=threads, decode=False, **hkw)))
            if one is None:
                one = got
                assert got == dev, (name, count, "the host's arrays are not the device's")
            assert got == one, (name, count, threads)
