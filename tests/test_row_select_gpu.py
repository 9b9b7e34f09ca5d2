"""Row selection, GPU part: lp_result_select on a device view (select.hip: an
ordered stream compaction of the status column), the dense tables
lp_result_table_rows / lp_result_table_map_rows (table.hip's row-list
instances) and the pseudo-columns @line / @offset / @lineno / @status.  Every
comparison is bit-exact: the device select against row_select_corpus.
expected_rows over r.status (the lp_line_status path) and against the host
copy's select; a dense table against the gather of the whole-batch device
table (pinned against the host and the oracle by test_gpu_parity /
test_table_map_gpu) and against the host replay of the same rows.  The CPU
part is test_row_select.py.

The select kernel's tiles in lines (csrc/kernels.h): a lane takes 16, a wave
W = SEL_WAVE_LINES = 1024, a block B = SEL_BLOCK_LINES = 4096.

The device-side bound check of a row list is deliberately not exercised here:
were it missing, the test would be an out-of-bounds read on a shared machine.
The host-copy test pins the return code."""
import collections
import ctypes
import functools
import re

import numpy as np
import pytest

import corpora
import logparser_amd as lpa
import row_select_corpus as rsc
import uri_wave_corpus as uwc

pytestmark = pytest.mark.gpu

W, B = lpa.SEL_WAVE_LINES, lpa.SEL_BLOCK_LINES
SIZES = (1, 63, 64, 65, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1)
REQ = "STRING:request.firstline.uri.query.*"
REF = "STRING:request.referer.query.*"
PSEUDO = [("@line", str), ("@offset", int), ("@lineno", int), ("@status", int)]
PATH, EPOCH, DATE = ("HTTP.PATH:request.firstline.uri.path", "TIME.EPOCH:request.receive.time.epoch",
                     "TIME.DATE:request.receive.time.date")  # DATE: formatted in k_table_chars again (SW_SLOW)
KIND = {str: lpa.CAST_STRING, int: lpa.CAST_LONG, float: lpa.CAST_DOUBLE}


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


@functools.lru_cache(None)
def _parser(fmt="combined"):
    """one handle per LogFormat for the whole module: every path of the format and the request's query wildcard"""
    return lpa.HttpdLoglineParser(fmt, [f for f in lpa.get_possible_paths(fmt) if not f.endswith("*")] + [REQ])


def _parse(lines_status, data=None, parser=None):
    lines = [l for l, _ in lines_status]
    r = (parser or _parser()).parse_batch(rsc.join_lf(lines) if data is None else data)
    assert r.n_lines == len(lines)
    assert r.status.tolist() == [s for _, s in lines_status]
    return r


def _view(r):
    v = lpa.LpResult()
    assert lpa.lib().lp_result_view(r._p._h, ctypes.byref(v)) == lpa.LP_OK
    return v


# ------------------------------------------------------------------ 1. select
def _check_select(r, res, first, count, mask):
    want = rsc.expected_rows(r.status, first, count, mask)
    got = r.select_device(mask, first, count)
    assert got.is_cuda and str(got.dtype) == "torch.int64"
    assert _np(got).tobytes() == want.tobytes(), (r.n_lines, first, count, mask)
    host = r.select_from(res, mask, first, count)
    assert host.dtype == np.int64 and host.tobytes() == want.tobytes(), (r.n_lines, first, count, mask, "host")


@pytest.mark.parametrize("pattern", ["ok", "none", "third", "mixed"])
def test_select_sizes_gpu(pattern):
    """batches of 1 .. 2B+1 lines (every wave / block boundary of the kernel
    and its neighbours), every mask 0..7, the whole batch"""
    for n in SIZES:
        r = _parse(rsc.pattern_lines(n, pattern))
        _, res = r.copy_to_host()
        for mask in range(8):
            _check_select(r, res, 0, n, mask)
        c = r.counters  # lp_counters are the exact sizes of a whole-batch select
        assert [len(r.select_device(m)) for m in (lpa.SEL_OK, lpa.SEL_BAD, lpa.SEL_FALLBACK)] == \
            [c["ok"], c["bad"], c["fallback"]]


def test_select_planted_gpu():
    r = _parse(rsc.planted())
    _, res = r.copy_to_host()
    for mask in range(8):
        _check_select(r, res, 0, r.n_lines, mask)
    assert set(r.status.tolist()) == {0, 1, 2}


def test_select_windows_gpu():
    """every first % 16 against counts around a lane's 16 lines and a wave's W;
    windows that end at the batch's last line; windows inside later blocks"""
    n = B + W + 57
    r = _parse(rsc.pattern_lines(n, "mixed"))
    _, res = r.copy_to_host()
    counts = (0, 1, 15, 16, 17, W, W + 1)
    for base in (0, B - 16):
        for f in range(16):
            for count in counts:
                for mask in (lpa.SEL_OK, lpa.SEL_BAD | lpa.SEL_FALLBACK, 7):
                    _check_select(r, res, base + f, count, mask)
    for count in counts + (n,):
        for mask in (lpa.SEL_OK, lpa.SEL_FALLBACK, 7):
            _check_select(r, res, n - count, count, mask)


def _raw_select(r, res, mask, cap, on_host, first=0, count=None):
    """one lp_result_select into a buffer of cap + 8 int64 words, every byte
    0x5A; returns (rc, rows_len, the buffer)"""
    import torch
    count = r.n_lines - first if count is None else count
    if on_host:
        buf = np.full(8 * (cap + 8), 0x5A, dtype=np.uint8).view(np.int64)
        ptr = buf.ctypes.data
    else:
        buf = torch.full((8 * (cap + 8),), 0x5A, dtype=torch.uint8, device="cuda").view(torch.int64)
        ptr = buf.data_ptr()
    n = ctypes.c_uint64(12345)
    rc = lpa.lib().lp_result_select(r._p._h, ctypes.byref(res), first, count, mask, ptr, cap, ctypes.byref(n))
    return rc, int(n.value), _np(buf)


@pytest.mark.parametrize("on_host", [False, True])
def test_select_size_protocol_gpu(on_host):
    r = _parse(rsc.pattern_lines(W + 65, "mixed"))
    hbuf, hres = r.copy_to_host()  # (hres points into hbuf)
    res = hres if on_host else _view(r)
    mask = lpa.SEL_OK | lpa.SEL_FALLBACK
    want = rsc.expected_rows(r.status, 0, r.n_lines, mask)
    need = len(want)
    assert need > W // 2
    sentinel = np.full(8, 0x5A, dtype=np.uint8).view(np.int64)[0]
    for cap in (0, need - 1):
        rc, n, buf = _raw_select(r, res, mask, cap, on_host)
        assert rc == lpa.LP_E_NOMEM and n == need, (cap, rc, n, need)
        assert (buf == sentinel).all(), cap  # nothing written, below the capacity or past it
    rc, n, buf = _raw_select(r, res, mask, need, on_host)
    assert rc == lpa.LP_OK and n == need
    assert buf[:need].tobytes() == want.tobytes() and (buf[need:] == sentinel).all()
    rc, n, buf = _raw_select(r, res, 0, 4, on_host)  # mask 0 selects nothing
    assert rc == lpa.LP_OK and n == 0 and (buf == sentinel).all()
    for bad_mask in (8, 1 << 31, 9):
        assert _raw_select(r, res, bad_mask, 4, on_host)[0] == lpa.LP_E_INVALID
    assert _raw_select(r, res, 7, 4, on_host, first=r.n_lines, count=1)[0] == lpa.LP_E_INVALID  # past the batch
    assert _raw_select(r, res, 7, 4, on_host, first=-1, count=1)[0] == lpa.LP_E_INVALID


# ------------------------------------------------------------- 2. dense table
def _whole_table(r, cols):
    return {p: ((tuple(_np(x) for x in v) if isinstance(v, tuple) else _np(v)), _np(ok))
            for p, (v, ok) in r.table_device(cols).items()}


def _check_rows_table(r, res, cols, whole, rows, what):
    """table_device(rows=) == the gather of the whole-batch table == table_from(rows=)"""
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    dev = r.table_device(cols, rows=_dev(rows))
    host = r.table_from(res, cols, rows=rows, threads=3, decode=False)
    for path, typ in cols:
        wv, wok = whole[path]
        dv, dok = dev[path]
        hv, hok = host[path]
        dok = _np(dok)
        assert dok.tolist() == wok[rows].tolist() == hok.astype(np.uint8).tolist(), (what, path)
        if path in lpa.PSEUDO_COLUMNS:
            assert dok.all(), (what, path)  # valid for every row, whatever its status
        if typ is str:
            off, chars, valid = rsc.gather_arrow(wv[0], wv[1], wok, rows)
            doff, dchars = _np(dv[0]), _np(dv[1])
            assert doff.tobytes() == off.tobytes(), (what, path)
            assert dchars.tobytes() == chars.tobytes(), (what, path)
            assert hv[0].tobytes() == off.tobytes() and hv[1][:off[-1]].tobytes() == chars.tobytes(), (what, path, "host")
        else:
            sel = dok.astype(bool)
            assert _np(dv)[sel].tobytes() == wv[rows][sel].tobytes() == hv[sel].tobytes(), (what, path)
    return dev


def _row_lists(r):
    import torch
    n = r.n_lines
    ok = _np(r.select_device(lpa.SEL_OK))
    not_ok = _np(r.select_device(lpa.SEL_BAD | lpa.SEL_FALLBACK))
    assert len(ok) > 64
    lists = {"ok": ok, "ok-reversed": ok[::-1], "repeats": np.repeat(ok[:40], 3)[5:], "empty": ok[:0],
             "not-ok-and-ok": np.concatenate([not_ok, ok[:9], not_ok[::-1]])}
    for length in (1, 63, 64, 65, 255, 256, 257):  # k_table_chars: a wave's 64 rows, a block's 256
        lists["len-%d" % length] = (np.arange(length, dtype=np.int64) * 37 + 11) % n
    assert isinstance(r.select_device(lpa.SEL_OK), torch.Tensor)
    return lists


@pytest.mark.parametrize("batch", ["planted", "config5"])
def test_dense_table_gpu(batch):
    """a STRING, a LONG, a formatted STRING (SW_SLOW), a query parameter and
    the four pseudo-columns in one call, over row lists in every order;
    config 5 (three LogFormats): fmt_id is indexed by line, not by row"""
    if batch == "planted":
        r = _parse(rsc.planted())
        param = "STRING:request.firstline.uri.query.a"
    else:
        p = _parser(lpa.SYNTH_FORMATS[lpa.SYNTH_MIXED])
        data = lpa.synth(lpa.SYNTH_MIXED, 5, 0, 3000)
        r = p.parse_batch(data)
        assert r.n_lines == 3000
        # the request parameter name the generator used most
        names = collections.Counter(n for u in re.findall(rb'"[A-Z]+ (\S+) HTTP', data) for n in re.findall(rb"[?&]([a-z0-9]+)=", u))
        param = "STRING:request.firstline.uri.query." + names.most_common(1)[0][0].decode()
    cols = [(PATH, str), (EPOCH, int), (DATE, str), (param, str)] + PSEUDO
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    whole = _whole_table(r, cols)
    assert whole[param][1].sum() > 0 and whole[DATE][1].sum() > 64
    for name, rows in _row_lists(r).items():
        dev = _check_rows_table(r, res, cols, whole, rows, (batch, name))
        if name == "ok":  # the dense table: every row has a record
            for path in (PATH, EPOCH, DATE):
                assert _np(dev[path][1]).tolist() == whole[path][1][rows].tolist()
            assert _np(dev[EPOCH][1]).all() and (_np(dev["@status"][0]) == lpa.LINE_OK).all()
        if name == "not-ok-and-ok" and batch == "planted":
            assert len(rows) > 100 and not _np(dev[PATH][1])[:8].any()  # a BAD / FALLBACK line's row: valid 0


# ---------------------------------------------------------- 3. pseudo-columns
def _split_arrow(off, chars):
    b = _np(chars).tobytes()
    off = _np(off)
    return [b[off[k]:off[k + 1]] for k in range(len(off) - 1)]


@pytest.mark.parametrize("variant", ["lf", "crlf", "lonecr", "unterminated"])
def test_pseudo_columns_gpu(variant):
    planted = rsc.planted()
    lines = [l for l, _ in planted]
    data = rsc.variants(lines)[variant]
    r = _parser().parse_batch(data)
    assert r.n_lines == len(lines)
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    dev = r.table_device(PSEUDO)
    host = r.table_from(res, PSEUDO, decode=False)
    for path, _ in PSEUDO:
        assert _np(dev[path][1]).all() and host[path][1].all(), path
    (off, chars), _ok = dev["@line"]
    got = _split_arrow(off, chars)
    assert got == corpora.split_hadoop(data) == lines  # the long line, the empty line, the invalid UTF-8
    assert _split_arrow(host["@line"][0][0], host["@line"][0][1][:int(host["@line"][0][0][-1])]) == lines
    offsets = [r.line_offset(i) for i in range(r.n_lines)]
    assert _np(dev["@offset"][0]).tolist() == offsets == host["@offset"][0].tolist()
    assert _np(dev["@status"][0]).tolist() == r.status.tolist() == host["@status"][0].tolist()
    first_line = _view(r).first_line
    assert _np(dev["@lineno"][0]).tolist() == [first_line + i for i in range(r.n_lines)] == host["@lineno"][0].tolist()
    # decoded: "@line" is bytes (its text is not validated), the row of a FALLBACK line included
    dec = r.table_from(res, [("@line", str)], rows=np.array([9, 11, 0], dtype=np.int64))["@line"][0]
    assert dec == [lines[9], b"", lines[0]]


def test_lineno_numbering_gpu():
    """@lineno on a handle's second batch and after lp_parse_batch_at"""
    p = lpa.HttpdLoglineParser("combined", [PATH])
    r1 = p.parse_batch(rsc.join_lf([l for l, _ in rsc.pattern_lines(70, "third")]))
    assert _np(r1.table_device([("@lineno", int)])["@lineno"][0]).tolist() == list(range(70))
    data = rsc.join_lf([l for l, _ in rsc.pattern_lines(130, "mixed")])
    r2 = p.parse_batch(data)
    assert _view(r2).first_line == 70
    rows = _dev([129, 0, 64])
    assert _np(r2.table_device([("@lineno", int)], rows=rows)["@lineno"][0]).tolist() == [199, 70, 134]
    L = lpa.lib()
    at = 1_000_000_007
    buf = ctypes.create_string_buffer(data, len(data))
    assert L.lp_parse_batch_at(p._h, ctypes.addressof(buf), len(data), at, lpa.BUF_HOST, None) == lpa.LP_OK
    assert L.lp_sync(p._h) == lpa.LP_OK
    r3 = lpa.BatchResult(p)
    assert _view(r3).first_line == at
    t = r3.table_device([("@lineno", int), ("@status", int)])
    assert _np(t["@lineno"][0]).tolist() == [at + i for i in range(130)]
    _, res = r3.copy_to_host()
    assert r3.table_from(res, [("@lineno", int)], rows=np.array([129, 1], np.int64))["@lineno"][0].tolist() == [at + 129, at + 1]


def _raw_table(r, res, specs, on_host, rows=None, n_rows=None, count=None, chars_cap=1 << 12):
    """one lp_result_table (rows None) / lp_result_table_rows call into
    buffers filled with 0x5A; specs: [(path, LP_CAST_*)]; rows: a pointer.
    Returns (rc, [{name: numpy}])"""
    import torch
    n = (count if rows is None else n_rows)
    mk = (lambda nb: np.full(nb, 0x5A, dtype=np.uint8)) if on_host else (
        lambda nb: torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda"))
    ptr = (lambda a: a.ctypes.data) if on_host else (lambda a: a.data_ptr())
    cols = (lpa.LpTableCol * len(specs))()
    bufs = []
    for k, (path, kind) in enumerate(specs):
        b = {"valid": mk(n + 8), "i64": mk(8 * (n + 2)), "f64": mk(8 * (n + 2)), "chars": mk(chars_cap)}
        bufs.append(b)
        c = cols[k]
        c.path, c.kind = path.encode(), kind
        c.valid, c.i64, c.f64, c.chars = ptr(b["valid"]), ptr(b["i64"]), ptr(b["f64"]), ptr(b["chars"])
        c.chars_cap = chars_cap
    L = lpa.lib()
    if rows is None:
        rc = L.lp_result_table(r._p._h, ctypes.byref(res), 0, n, cols, len(specs), 2)
    else:
        rc = L.lp_result_table_rows(r._p._h, ctypes.byref(res), rows, n, cols, len(specs), 2)
    return rc, [{k: _np(v) for k, v in b.items()} for b in bufs]


def _untouched(bufs):
    return all((a == 0x5A).all() for b in bufs for a in b.values())


@pytest.mark.parametrize("on_host", [False, True])
def test_pseudo_column_kinds_gpu(on_host):
    r = _parse(rsc.pattern_lines(5, "mixed"))
    hbuf, hres = r.copy_to_host()  # (hres points into hbuf)
    res = hres if on_host else _view(r)
    S, I, D = lpa.CAST_STRING, lpa.CAST_LONG, lpa.CAST_DOUBLE
    for path, kind in (("@line", I), ("@line", D), ("@offset", S), ("@lineno", S), ("@status", S), ("@status", D)):
        rc, bufs = _raw_table(r, res, [(path, kind)], on_host, count=5)
        assert rc == lpa.LP_E_INVALID and _untouched(bufs), (path, kind, rc)
    rc, _ = _raw_table(r, res, [("@nothing", S)], on_host, count=5)
    assert rc == lpa.LP_E_MISSING
    rc, bufs = _raw_table(r, res, [("@line", S), ("@offset", I), ("@lineno", I), ("@status", I)], on_host, count=5)
    assert rc == lpa.LP_OK
    assert bufs[3]["i64"].view(np.int64)[:5].tolist() == r.status.tolist()


# --------------------------------------------------------------- 4. dense map
@functools.lru_cache(None)
def _piece_case():
    return uwc.piece_cases()[-1]


def _same_arrays(got, want, what):
    for n in lpa.MAP_ARRAYS:
        g, w = _np(got[n]), _np(want[n])
        assert g.shape == w.shape, (what, n, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, n)


def test_dense_map_gpu():
    """a 300-piece line, piece totals across 64: REQ and REF over row lists"""
    c = _piece_case()
    p = lpa.HttpdLoglineParser("combined", [REQ, REF])
    r = p.parse_batch(c.data)
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    whole = {k: {n: _np(a) for n, a in v.items()} for k, v in r.table_map_device([REQ, REF], decode=False).items()}
    ok = _np(r.select_device(lpa.SEL_OK))
    assert len(ok) == r.n_lines > 64 and np.diff(whole[REQ]["entry_off"]).max() >= 8
    lists = {"ok": ok, "reversed": ok[::-1], "repeats": np.repeat(ok[:70], 2)[3:], "empty": ok[:0],
             "scattered": (np.arange(257, dtype=np.int64) * 29 + 3) % r.n_lines}
    for name, rows in lists.items():
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        dev = r.table_map_device([REQ, REF], rows=_dev(rows), decode=False)
        host = r.table_map_from(res, [REQ, REF], rows=rows, threads=3, decode=False)
        for path in (REQ, REF):
            want = rsc.gather_map(whole[path], rows)
            _same_arrays(dev[path], want, ("device", name, path))
            _same_arrays(host[path], want, ("host", name, path))
    # decoded rows: the same dicts as the whole batch's
    maps = r.table_map_device([REQ])[REQ]
    assert r.table_map_device([REQ], rows=_dev(ok[::-1][:20]))[REQ] == [maps[i] for i in ok[::-1][:20]]


def test_dense_map_size_protocol_gpu():
    """each of the three capacities one short: LP_E_NOMEM with the exact lengths"""
    import torch
    c = _piece_case()
    p = lpa.HttpdLoglineParser("combined", [REQ])
    r = p.parse_batch(c.data)
    res = _view(r)
    rows = np.ascontiguousarray(_np(r.select_device(lpa.SEL_OK))[::-1][:150])
    whole = {n: _np(a) for n, a in r.table_map_device([REQ], decode=False)[REQ].items()}
    want = rsc.gather_map(whole, rows)
    need = (len(want["key_off"]) - 1, len(want["key_chars"]), len(want["val_chars"]))
    assert min(need) > 64, need
    d_rows = _dev(rows)
    n = len(rows)

    def call(caps):
        mk = lambda cnt, dt: torch.full((cnt * np.dtype(dt).itemsize,), 0x5A, dtype=torch.uint8, device="cuda").view(
            {np.uint8: torch.uint8, np.int64: torch.int64}[dt])
        b = {"valid": mk(n + 8, np.uint8), "entry_off": mk(n + 2, np.int64), "key_off": mk(caps[0] + 2, np.int64),
             "val_off": mk(caps[0] + 2, np.int64), "key_chars": mk(caps[1] + 8, np.uint8), "val_chars": mk(caps[2] + 8, np.uint8)}
        col = lpa.LpTableMapCol()
        col.path = REQ.encode()
        for name in lpa.MAP_ARRAYS:
            setattr(col, name, b[name].data_ptr())
        col.entries_cap, col.key_chars_cap, col.val_chars_cap = caps
        rc = lpa.lib().lp_result_table_map_rows(p._h, ctypes.byref(res), d_rows.data_ptr(), n, ctypes.byref(col), 1, 0)
        return rc, (int(col.entries_len), int(col.key_chars_len), int(col.val_chars_len)), {k: _np(a) for k, a in b.items()}

    for short in range(3):
        caps = tuple(x - (1 if k == short else 0) for k, x in enumerate(need))
        rc, got, _b = call(caps)
        assert rc == lpa.LP_E_NOMEM and got == need, (short, rc, got, need)
    rc, got, b = call(need)
    assert rc == lpa.LP_OK and got == need
    for name, used in (("valid", n), ("entry_off", n + 1), ("key_off", need[0] + 1), ("val_off", need[0] + 1),
                       ("key_chars", need[1]), ("val_chars", need[2])):
        assert b[name][:used].tobytes() == want[name].tobytes(), name
        assert (b[name].view(np.uint8)[used * b[name].itemsize:] == 0x5A).all(), name


# -------------------------------------------------------------------- 5. reuse
def test_reused_handle_and_buffers_gpu():
    """one handle, one rows buffer and one set of table buffers prefilled with
    0xA5, two different batches: select plus dense table each time; nothing
    stale is read or left"""
    import torch
    p = lpa.HttpdLoglineParser("combined", lpa.get_possible_paths("combined"))
    cols = [(PATH, str), (EPOCH, int), (DATE, str), ("@line", str), ("@lineno", int)]
    rows_buf = torch.empty(4096, dtype=torch.int64, device="cuda")
    bufs = None
    first_line = 0
    for k, ls in enumerate((rsc.planted(), rsc.pattern_lines(300, "mixed"), rsc.planted())):
        r = _parse(ls, parser=p)
        if bufs is None:
            bufs = r.table_buffers(cols, count=4096, chars_cap=1 << 20)
            keep = [list(b) for b in bufs]
        rows_buf.view(torch.uint8).fill_(0xA5)
        for b in bufs:
            for t in b:
                if t is not None:
                    t.view(torch.uint8).fill_(0xA5)
        n = ctypes.c_uint64(0)
        mask = lpa.SEL_OK if k != 1 else lpa.SEL_OK | lpa.SEL_FALLBACK
        view = _view(r)
        rc = lpa.lib().lp_result_select(p._h, ctypes.byref(view), 0, r.n_lines, mask, rows_buf.data_ptr(), 4096,
                                        ctypes.byref(n))
        want = rsc.expected_rows(r.status, 0, r.n_lines, mask)
        assert rc == lpa.LP_OK and n.value == len(want)
        assert _np(rows_buf[:len(want)]).tobytes() == want.tobytes()
        assert (_np(rows_buf[len(want):].view(torch.uint8)) == 0xA5).all()
        dev = r.table_device(cols, buffers=bufs, rows=rows_buf[:len(want)])
        assert all(x is y for b, kb in zip(bufs, keep) for x, y in zip(b, kb)), "a buffer was too small"
        hbuf, res = r.copy_to_host()  # (res points into hbuf)
        host = r.table_from(res, cols, rows=want, decode=False)
        for path, typ in cols:
            dv, dok = dev[path]
            hv, hok = host[path]
            assert _np(dok).tolist() == hok.astype(np.uint8).tolist(), (k, path)
            if typ is str:
                assert _np(dv[0]).tobytes() == hv[0].tobytes(), (k, path)
                assert _np(dv[1]).tobytes() == hv[1][:hv[0][-1]].tobytes(), (k, path)
            else:
                assert _np(dv)[hok].tobytes() == hv[hok].tobytes(), (k, path)
        lines = [l for l, _ in ls]
        assert _split_arrow(*dev["@line"][0]) == [lines[i] for i in want]
        assert _np(dev["@lineno"][0]).tolist() == (first_line + want).tolist()
        first_line += r.n_lines


# ------------------------------------------------------------------- 6. errors
def test_errors_gpu():
    p = lpa.HttpdLoglineParser("combined", [PATH, REQ])
    r = _parse(rsc.pattern_lines(80, "mixed"), parser=p)
    hbuf, hres = r.copy_to_host()  # (hres points into hbuf)
    view = _view(r)
    S, I = lpa.CAST_STRING, lpa.CAST_LONG
    specs = [(PATH, S), ("@offset", I), ("@line", S)]
    # host copy: an index outside [0, n_lines) is refused before anything is written
    for bad in (-1, 80, 1 << 40):
        rows = np.array([3, 0, bad, 5], dtype=np.int64)
        rc, bufs = _raw_table(r, hres, specs, True, rows=rows.ctypes.data, n_rows=4)
        assert rc == lpa.LP_E_INVALID and _untouched(bufs), bad
        with pytest.raises(ValueError):
            r.table_map_from(hres, [REQ], rows=rows)
    rows = np.array([3, 0, 79, 5], dtype=np.int64)
    rc, bufs = _raw_table(r, hres, specs, True, rows=rows.ctypes.data, n_rows=4)
    assert rc == lpa.LP_OK and bufs[1]["i64"].view(np.int64)[:4].tolist() == [r.line_offset(int(i)) for i in rows]
    assert _raw_table(r, hres, specs, True, rows=None, n_rows=None, count=81)[0] == lpa.LP_E_INVALID
    L = lpa.lib()
    col = lpa.LpTableCol()
    assert L.lp_result_table_rows(p._h, ctypes.byref(hres), None, 3, ctypes.byref(col), 1, 1) == lpa.LP_E_INVALID
    assert L.lp_result_table_rows(p._h, ctypes.byref(hres), rows.ctypes.data, -1, ctypes.byref(col), 1, 1) == lpa.LP_E_INVALID
    # a device view takes device rows only: host memory is refused, never dereferenced
    rc, bufs = _raw_table(r, view, specs, False, rows=rows.ctypes.data, n_rows=4)
    assert rc in (lpa.LP_E_INVALID, lpa.LP_E_STATE) and _untouched(bufs)
    with pytest.raises(ValueError):
        r.table_device([(PATH, str)], rows=rows)  # (the mirror refuses a numpy array there too)
    with pytest.raises(ValueError):
        r.table_device([(PATH, str)], rows=_dev(rows), first=1)
    with pytest.raises(ValueError):
        r.table_map_device([REQ], rows=_dev(rows), count=2)
    n = ctypes.c_uint64(0)
    out = np.zeros(128, dtype=np.int64)
    assert L.lp_result_select(p._h, ctypes.byref(view), 0, 80, 7, out.ctypes.data, 128, ctypes.byref(n)) in (
        lpa.LP_E_INVALID, lpa.LP_E_STATE)
    assert not out.any()
    # a view of an older batch
    r2 = _parse(rsc.pattern_lines(33, "third"), parser=p)
    d_rows = _dev([1, 2])
    rc, bufs = _raw_table(r2, view, specs, False, rows=d_rows.data_ptr(), n_rows=2)
    assert rc in (lpa.LP_E_STATE, lpa.LP_E_INVALID) and _untouched(bufs)
    rc, _n, buf = _raw_select(r2, view, 7, 128, False, first=0, count=33)
    assert rc in (lpa.LP_E_STATE, lpa.LP_E_INVALID) and (buf.view(np.uint8) == 0x5A).all()
    mcol = lpa.LpTableMapCol()
    assert L.lp_result_table_map_rows(p._h, ctypes.byref(view), d_rows.data_ptr(), 2, ctypes.byref(mcol), 1, 0) in (
        lpa.LP_E_STATE, lpa.LP_E_INVALID)
    # the new batch's own view works
    got = r2.table_device([("@status", int)], rows=d_rows)["@status"][0]
    assert _np(got).tolist() == r2.status[[1, 2]].tolist()
