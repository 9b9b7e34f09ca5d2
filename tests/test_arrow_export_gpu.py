"""Arrow C Data Interface export, GPU part: lp_result_arrow on a device view
(arrow.hip: k_arrow_validity packs the validity bitmaps and counts the nulls of
every column in one launch, k_arrow_narrow32 narrows a map's entry offsets) and
lp_arrow_from_tables on device buffers.  The truth is the device's own existing
tables over the same rows (table_device, table_dict_device, table_map_device:
pinned against the host replay and the oracle by the other GPU files); a device
export copied to the host equals the export of a host copy (RecordBatch.equals),
and pyarrow validates both fully.  The CPU part is test_arrow_export.py.

The validity kernel's tiles in rows (csrc/kernels.h): a lane takes 16, a wave
W = ARROW_WAVE_ROWS = 1024, a block B = ARROW_BLOCK_ROWS = 4096.

Formats: the combined corpora deliver no DOUBLE column (the one DOUBLE cast the
formats have is a SECOND_MILLIS list item of the NGINX format), so the DOUBLE
column is checked on config 5, over windows of its own.

As in test_row_select_gpu.py, a row index outside the batch is not exercised on
the device: were the kernels' bound check missing, the test would be an
out-of-bounds read on a shared machine."""
import collections
import ctypes
import functools
import re

import numpy as np
import pyarrow as pa  # noqa: F401
import pytest

import arrow_corpus as ac
import dict_corpus as dc
import logparser_amd as lpa
import row_select_corpus as rsc
import uri_wave_corpus as uwc

pytestmark = pytest.mark.gpu

W, B = lpa.ARROW_WAVE_ROWS, lpa.ARROW_BLOCK_ROWS
WINDOWS = (0, 1, 15, 16, 17, 63, 64, 65, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1)
REQ = "STRING:request.firstline.uri.query.*"
REF = "STRING:request.referer.query.*"
PATH, EPOCH, DATE = ("HTTP.PATH:request.firstline.uri.path", "TIME.EPOCH:request.receive.time.epoch",
                     "TIME.DATE:request.receive.time.date")
PARAM_A = "STRING:request.firstline.uri.query.a"
PSEUDO = [("@line", str), ("@offset", int), ("@lineno", int), ("@status", int)]
# every column form in one call: a STRING, a LONG, a formatted STRING, a query parameter, the four
# pseudo-columns, a dictionary column (under a field name of its own), a map column
COLS = [(PATH, str), (EPOCH, int), (DATE, str), (PARAM_A, str)] + PSEUDO + [(dc.UA, "dict", "ua"), (REQ, "map")]
SECMS = "SECOND_MILLIS:nginxmodule.upstream.response.time.0.value"


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


@functools.lru_cache(None)
def _parser(fmt="combined"):
    """one handle per LogFormat for the whole module: every path of the format and the request's query wildcard"""
    return lpa.HttpdLoglineParser(fmt, [f for f in lpa.get_possible_paths(fmt) if not f.endswith("*")] + [REQ])


def _parse(lines_status, parser=None):
    lines = [l for l, _ in lines_status]
    r = (parser or _parser()).parse_batch(rsc.join_lf(lines))
    assert r.n_lines == len(lines) and r.status.tolist() == [s for _, s in lines_status]
    return r


def _name(col):
    return col[2] if len(col) > 2 else col[0]


def _truth(r, cols, first=0, count=None, rows=None):
    """{field name: the values RecordBatch.to_pylist must show} from the device's existing tables"""
    kw = dict(rows=rows) if rows is not None else dict(first=first, count=count)
    out = {}
    plain = [c for c in cols if c[1] in (str, int, float)]
    if plain:
        t = r.table_device([(c[0], c[1]) for c in plain], **kw)
        for c in plain:
            data, valid = t[c[0]]
            data = tuple(_np(a) for a in data) if c[1] is str else _np(data)
            out[_name(c)] = ac.plain_pylist(c[1], _np(valid), data, binary=c[0] == "@line")
    for c in cols:
        if c[1] == "dict":
            index, (doff, dchars), valid = r.table_dict_device([c[0]], **kw)[c[0]]
            out[_name(c)] = lpa.strings_from_dict(_np(valid), _np(index), _np(doff), _np(dchars))
        elif c[1] == "map":
            rows_of = r.table_map_device([c[0]], **kw)[c[0]]
            out[_name(c)] = [None if d is None else list(d.items()) for d in rows_of]
    return out


def _check(r, res, cols, first=0, count=None, rows=None, what=None):
    """device export -> host equals the host copy's export, both equal the device tables' decode;
    returns the device export (the caller releases it)"""
    e = r.to_arrow_device(cols, first, count, rows=rows)
    got = e.to_host()
    host = r.to_arrow(res, cols, first, count, rows=None if rows is None else _np(rows))
    want = _truth(r, cols, first, count, rows)
    n = len(next(iter(want.values())))
    for b in (got, host):
        b.validate(full=True)
        assert b.num_rows == n and b.schema.names == [_name(c) for c in cols], what
    assert got.equals(host), what
    assert got.schema.equals(host.schema), what
    for name, vals in want.items():
        assert got.column(name).to_pylist() == vals, (what, name)
    return e


# ---------------------------------------------------------------- 1. windows
@pytest.mark.parametrize("pattern", ["ok", "none", "third", "planted"])
def test_window_tiles_gpu(pattern):
    """windows of 0 .. 2B+1 rows (every lane / wave / block boundary of the validity kernel and its
    neighbours) of batches that are all OK, without an OK line, every third BAD, and the planted mix"""
    if pattern == "planted":
        r = _parse(rsc.planted())
    else:
        r = _parse(rsc.pattern_lines(2 * B + 1 + 3, pattern))
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    for size in WINDOWS:
        if size > r.n_lines:
            continue
        first = 3 if size and size + 3 <= r.n_lines else 0
        e = _check(r, res, COLS, first, size, what=(pattern, first, size))
        top = e.device_array.array
        assert top.length == size and top.null_count == 0 and top.n_children == len(COLS)
        pseudo = [ac.child(top, k) for k in range(4, 8)]
        assert all(c.null_count == 0 and ac.buffer_ptr(c, 0) is None for c in pseudo)  # valid for every row
        if pattern == "ok":  # no nulls anywhere: no bitmap at all
            assert all(ac.child(top, k).null_count == 0 and ac.buffer_ptr(ac.child(top, k), 0) is None for k in range(len(COLS)))
        if pattern == "none" and size:
            assert ac.child(top, 0).null_count == size and ac.child(top, 9).null_count == size
        e.release()
    assert r.arrow_timing() > 0


def test_config5_double_and_formats_gpu():
    """config 5 (three LogFormats): the DOUBLE of a SECOND_MILLIS list item beside the other forms;
    rows of a LogFormat that does not deliver a path are nulls (a map: valid and empty)"""
    p = _parser(lpa.SYNTH_FORMATS[lpa.SYNTH_MIXED])
    data = lpa.synth(lpa.SYNTH_MIXED, 5, 0, 3000)
    r = p.parse_batch(data)
    assert r.n_lines == 3000
    names = collections.Counter(n for u in re.findall(rb'"[A-Z]+ (\S+) HTTP', data) for n in re.findall(rb"[?&]([a-z0-9]+)=", u))
    param = "STRING:request.firstline.uri.query." + names.most_common(1)[0][0].decode()
    cols = [(SECMS, float, "upstream_s"), (PATH, str), (EPOCH, int), (DATE, str), (param, str)] + PSEUDO + \
           [("HTTP.USERAGENT:request.user-agent", "dict"), (REQ, "map", "query")]
    hbuf, res = r.copy_to_host()
    for first, count in ((0, 3000), (1, W + 1), (1500, 65), (2999, 1), (17, 0)):
        e = _check(r, res, cols, first, count, what=("config5", first, count))
        if count == 3000:
            rb = e.to_host()
            dbl = rb.column("upstream_s")
            assert str(dbl.type) == "double" and 0 < dbl.null_count < 3000
            assert any(m == [] for m in rb.column("query").to_pylist())
        e.release()


# ------------------------------------------------------------ 2. raw bitmaps
def _raw_host(e):
    """lp_arrow_to_host itself: the host ArrowArray of a deep copy (buffers byte for byte), to release"""
    return e.to_host_array()


def test_raw_bitmaps_of_an_export_gpu():
    """the raw device bitmap equals packbits of the device table's valid bytes, padding included"""
    r = _parse(rsc.pattern_lines(B + W + 57, "mixed"))
    for first, count in ((0, r.n_lines), (5, W + 9), (B - 7, 130), (0, 7)):
        t = r.table_device([(PATH, str), (PARAM_A, str)], first, count)
        m = r.table_map_device([REQ], first, count, decode=False)[REQ]
        e = r.to_arrow_device([(PATH, str), (PARAM_A, str), (REQ, "map")], first, count)
        raw = _raw_host(e)
        for k, valid in enumerate((_np(t[PATH][1]), _np(t[PARAM_A][1]), _np(m["valid"]))):
            col = ac.child(raw, k)
            assert 0 < col.null_count == int((valid == 0).sum())
            got = ac.host_bytes(col, 0, ac.bitmap_bytes(count))
            assert np.array_equal(got, ac.expected_bitmap(valid)), (first, count, k)
        off32 = ac.host_bytes(ac.child(raw, 2), 1, 4 * (count + 1)).view(np.int32)
        assert np.array_equal(off32, _np(m["entry_off"]).astype(np.int32))
        raw.release(ctypes.byref(raw))
        e.release()


@pytest.mark.parametrize("n", ac.BITMAP_SIZES)
def test_from_tables_bitmaps_and_skews_gpu(n):
    """lp_arrow_from_tables on torch buffers: sixteen columns in one launch whose valid bytes start at
    byte skews 0..15; every byte around the rows is 0xA5, so a read outside [0, n) would show as
    padding bits; every pattern of the CPU test; the values buffers are wrapped, not copied"""
    import torch
    for name in ac.PATTERNS:
        pools = [torch.full((n + 512,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(16)]
        values = torch.arange(max(1, n), dtype=torch.int64, device="cuda")
        valids, views = [], []
        for skew in range(16):
            v = ac.pattern(name, n, seed=skew)
            assert pools[skew].data_ptr() % 256 == 0
            view = pools[skew][256 + skew:256 + skew + n]
            view.copy_(torch.from_numpy(v))
            valids.append(v)
            views.append(view)
        assert n == 0 or len({v.data_ptr() % 16 for v in views}) == 16
        calls = []
        e = lpa.arrow_from_tables(n, plain=[("c%d" % s, int, views[s], values) for s in range(16)], device=0,
                                  on_release=lambda: calls.append(1))
        d = e.device_array
        assert (d.device_type, d.device_id, d.sync_event) == (lpa.ARROW_DEVICE_ROCM, 0, None)
        raw = _raw_host(e)
        for s in range(16):
            col, dcol = ac.child(raw, s), ac.child(d.array, s)
            nulls = int((valids[s] == 0).sum())
            assert col.length == n and col.null_count == nulls == dcol.null_count, (n, name, s)
            assert ac.buffer_ptr(dcol, 1) == values.data_ptr()  # wrapped
            if nulls == 0:
                assert ac.buffer_ptr(dcol, 0) is None and ac.buffer_ptr(col, 0) is None
            else:
                got = ac.host_bytes(col, 0, ac.bitmap_bytes(n))
                assert np.array_equal(got, ac.expected_bitmap(valids[s])), (n, name, s, np.flatnonzero(got != ac.expected_bitmap(valids[s]))[:8])
        raw.release(ctypes.byref(raw))
        assert calls == []
        e.release()
        assert calls == [1]


# -------------------------------------------------------------- 3. row lists
def test_row_lists_gpu():
    """the OK rows (no nulls: every validity pointer NULL), reversed, with repeats, empty, and lists of
    1, 63, 64, 65, 1025 rows"""
    r = _parse(rsc.planted())
    hbuf, res = r.copy_to_host()
    ok = r.select_device(lpa.SEL_OK)
    n = r.n_lines
    e = _check(r, res, COLS, rows=ok, what="ok")
    top = e.device_array.array
    assert top.length == len(ok) > 100
    for k in range(len(COLS)):
        assert ac.child(top, k).null_count == 0 and ac.buffer_ptr(ac.child(top, k), 0) is None, COLS[k]
    e.release()
    lists = {"reversed": np.arange(n)[::-1], "repeats": np.repeat(np.arange(0, n, 3), 2), "empty": np.zeros(0, np.int64)}
    for L in (1, 63, 64, 65, 1025):
        lists["len%d" % L] = (np.arange(L) * 7 + 5) % n
    for name, rows in lists.items():
        _check(r, res, COLS, rows=_dev(rows), what=name).release()


def test_map_row_gathered_twice_gpu():
    """the 300-piece line gathered twice: the narrowed offsets are entry_off as int32"""
    c = uwc.piece_cases()[-1]
    p = lpa.HttpdLoglineParser("combined", [REQ, REF])
    r = p.parse_batch(c.data)
    hbuf, res = r.copy_to_host()
    per_row = np.diff(_np(r.table_map_device([REQ], decode=False)[REQ]["entry_off"]))
    # (a 300-piece line: 200 pieces in its request query; its keys repeat, so the surviving entries are the distinct keys)
    big = max(range(len(c.lines)), key=lambda i: len(c.lines[i]))
    assert c.lines[big].count(b"&") >= 199 and per_row[big] == per_row.max() >= 8
    rows = _dev([big, 0, big, 1, big])
    cols = [(REQ, "map"), (REF, "map", "referer"), ("@lineno", int)]
    e = _check(r, res, cols, rows=rows, what="big map row")
    want = _np(r.table_map_device([REQ], rows=rows, decode=False)[REQ]["entry_off"])
    raw = _raw_host(e)
    m = ac.child(raw, 0)
    assert ac.child(m, 0).length == int(want[-1]) >= 3 * per_row[big]
    assert np.array_equal(ac.host_bytes(m, 1, 4 * 6).view(np.int32), want.astype(np.int32))
    raw.release(ctypes.byref(raw))
    e.release()


# --------------------------------------------------------------- 4. lifetime
def test_export_outlives_later_batches_and_the_parser_gpu():
    p = lpa.HttpdLoglineParser("combined", [f for f in lpa.get_possible_paths("combined") if not f.endswith("*")] + [REQ])
    r = p.parse_batch(rsc.join_lf([l for l, _ in rsc.planted()]))
    e = r.to_arrow_device(COLS)
    first = e.to_host()
    first.validate(full=True)
    # two further, different batches on the same handle: the handle's own buffers are rewritten
    p.parse_batch(rsc.join_lf([l for l, _ in rsc.pattern_lines(3000, "mixed")]))
    p.parse_batch(rsc.join_lf([dc.line(k) for k in range(500)]))
    again = e.to_host()
    again.validate(full=True)
    assert again.equals(first)
    # the handle itself goes
    p._close()
    last = e.to_host()
    last.validate(full=True)
    assert last.equals(first) and last.num_rows == 200
    e.release()
    assert not e.device_array.array.release


# --------------------------------------------------------------- 5. refusals
def test_refusals_gpu():
    """host-memory rows on a device view: LP_E_INVALID; an older batch's view: LP_E_STATE; a path the
    device table does not derive: LP_E_UNSUPPORTED, passed through; both outputs released each time"""
    r = _parse(rsc.planted())
    view = r._view()
    host_rows = np.arange(10, dtype=np.int64)
    rc, schema, dev = r.arrow_call(view, COLS, 0, 10, rows_p=host_rows.ctypes.data)
    assert rc == lpa.LP_E_INVALID and ac.released(schema, dev)
    rc, schema, dev = r.arrow_call(view, [(PATH, str), ("@status", 7)], 0, 10)
    assert rc == lpa.LP_E_INVALID and ac.released(schema, dev)
    rc, schema, dev = r.arrow_call(view, [("STRING:request.no.such.path", str)], 0, 10)
    assert rc == lpa.LP_E_MISSING and ac.released(schema, dev)
    _parse(rsc.pattern_lines(77, "third"))  # the handle's next batch: the view is an older batch's
    rc, schema, dev = r.arrow_call(view, COLS, 0, 10)
    assert rc == lpa.LP_E_STATE and ac.released(schema, dev)
    # a remapped delivery itself: only the host replay derives it
    num = "NUM:request.firstline.uri.query.a"
    q = lpa.HttpdLoglineParser(dc.FMT, [num, PATH])
    q.add_type_remapping("request.firstline.uri.query.a", "NUM", lpa.STRING_OR_LONG_OR_DOUBLE)
    rq = q.parse_batch(dc.join_lf([dc.line(k) for k in range(130)]))
    rc, schema, dev = rq.arrow_call(rq._view(), [(PATH, str), (num, str)], 0, 130)
    assert rc == lpa.LP_E_UNSUPPORTED and ac.released(schema, dev)
    with pytest.raises(lpa.FallbackRequired):
        rq.to_arrow_device([(num, "dict")])
    hbuf, res = rq.copy_to_host()
    rb = rq.to_arrow(res, [(PATH, str), (num, str)])  # the host copy answers
    rb.validate(full=True)
    assert rb.num_rows == 130 and rb.column(num).null_count == 0


# ---------------------------------------------------------- 6. device fields
def _device_pointers(array, out):
    for k in range(array.n_buffers):
        if array.buffers[k]:
            out.append(array.buffers[k])
    for k in range(array.n_children):
        _device_pointers(array.children[k].contents, out)
    if array.dictionary:
        _device_pointers(array.dictionary.contents, out)
    return out


def test_device_fields_gpu():
    """ARROW_DEVICE_ROCM, the handle's device, no sync event; every buffer is device memory"""
    import torch
    r = _parse(rsc.planted())
    e = r.to_arrow_device(COLS, 0, 130)
    d = e.device_array
    assert d.device_type == 10 == lpa.ARROW_DEVICE_ROCM and d.device_id == r._p.device and not d.sync_event
    assert list(d.reserved) == [0, 0, 0] and e.on_device
    ptrs = _device_pointers(d.array, [])
    assert len(ptrs) >= 2 * len(COLS)
    hip = ctypes.CDLL(torch.__path__[0] + "/lib/libamdhip64.so")

    class Attr(ctypes.Structure):  # hipPointerAttribute_t
        _fields_ = [("type", ctypes.c_int), ("device", ctypes.c_int), ("devicePointer", ctypes.c_void_p),
                    ("hostPointer", ctypes.c_void_p), ("isManaged", ctypes.c_int), ("allocationFlags", ctypes.c_uint)]
    for p in ptrs:
        a = Attr()
        assert hip.hipPointerGetAttributes(ctypes.byref(a), ctypes.c_void_p(p)) == 0
        assert a.type == 2 and a.device == r._p.device, hex(p)  # hipMemoryTypeDevice
    with pytest.raises(ValueError):
        e.record_batch()  # device memory is not importable as a host batch
    e.release()
