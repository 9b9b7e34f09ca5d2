"""lp_result_table_map (a wildcard target as an Arrow map<string,string>
column), GPU part: the column built in HBM (table.hip: k_map_count,
k_map_entries, k_map_fill, k_map_chars) equals the host replay's byte for
byte, and both equal the maps derived from the oracle's records
(table_map_ref) on every line.  The CPU part is test_table_map.py."""
import ctypes
import functools

import numpy as np
import pytest

import logparser_amd as lpa
import table_map_ref as tmr
import uri_wave_corpus as uwc

pytestmark = pytest.mark.gpu

REQ = "STRING:request.firstline.uri.query.*"
REF = "STRING:request.referer.query.*"
HEAD = b'1.2.3.4 - - [10/Oct/2026:13:55:36 +0200] "GET %s HTTP/1.1" 200 5 "%s" "ua"'


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _same_arrays(dev, host, what):
    for p in host:
        for n in lpa.MAP_ARRAYS:
            d, h = _np(dev[p][n]), _np(host[p][n])
            assert d.shape == h.shape, (what, p, n, d.shape, h.shape)
            assert d.tobytes() == h.tobytes(), (what, p, n, int(np.argmax(d != h)))


def check(oracle, key, fmt, fields, lines, paths, data=None, remaps=(), parser=None, threads=5):
    """device == host == oracle on one batch; returns (batch, host arrays)"""
    p = parser or lpa.HttpdLoglineParser(fmt, fields)
    r = p.parse_batch(b"".join(l + b"\n" for l in lines) if data is None else data)
    assert r.n_lines == len(lines), (key, r.n_lines)
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    host = r.table_map_from(res, paths, threads=threads, decode=False)
    dev = r.table_map_device(paths, decode=False)
    _same_arrays(dev, host, key)
    ref = tmr.oracle_maps(oracle, key, fmt, fields, lines, paths, remaps)
    for path in paths:
        a = host[path]
        maps = lpa.maps_from_arrow(*(a[n] for n in lpa.MAP_ARRAYS))
        per_row = np.diff(a["entry_off"])
        for i in range(r.n_lines):
            if r.status[i] != lpa.LINE_OK:  # BAD, FALLBACK: no record, no entries
                assert maps[i] is None and per_row[i] == 0, (key, path, i, lines[i])
                assert r.status[i] == lpa.LINE_FALLBACK or ref[i] is None, (key, i)
                continue
            assert ref[i] is not None and maps[i] == ref[i][path], (key, path, i, lines[i], maps[i], ref[i][path])
            assert per_row[i] == len(maps[i]), (key, path, i)  # one entry per key
    return r, host


@functools.lru_cache(None)
def _piece_cases():
    return uwc.piece_cases()


def test_handwritten_order_gpu(oracle):
    """The order the project fixes: a surviving entry stands at the position
    of its last delivery.  ?a=1&A=2&b&a=3&=x&&c=%41 -> b, a, "", c."""
    lines = [HEAD % (b"/p?a=1&A=2&b&a=3&=x&&c=%41", b"http://h/r?Z=1&z=&y"), HEAD % (b"/p", b"-"), b"garbage",
             HEAD % (b"/p?x=1&x=2&x=3", b"http://h/?q=%41+b&Q")]
    r, host = check(oracle, "hand", "combined", [REQ, REF], lines, [REQ, REF])
    req = lpa.maps_from_arrow(*(host[REQ][n] for n in lpa.MAP_ARRAYS))
    ref = lpa.maps_from_arrow(*(host[REF][n] for n in lpa.MAP_ARRAYS))
    assert list(req[0].items()) == [("b", ""), ("a", "3"), ("", "x"), ("c", "A")]
    assert list(ref[0].items()) == [("z", ""), ("y", "")]
    assert req[1] == {} and ref[1] == {} and req[2] is None and ref[2] is None
    assert list(req[3].items()) == [("x", "3")] and list(ref[3].items()) == [("q", "")]
    assert r.table_map_device([REQ])[REQ] == req


def test_piece_corpus_gpu(oracle):
    """E: wave piece totals 1..8, every ~37 up to ~700, every multiple of 64
    and its neighbours, lines of up to 200 + 100 pieces (request + referer):
    both query wildcards in one call."""
    from test_gpu_parity import paths
    for c in _piece_cases():
        r, _ = check(oracle, c.name, "combined", paths(oracle), c.lines, [REQ, REF], data=c.data)
        assert r.counters["ok"] == len(c.lines)


@pytest.mark.parametrize("kind", ["cookie", "querystring", "setcookie"])
def test_pair_stage_corpora_gpu(oracle, kind):
    """The pair stages: request cookies, a raw %q query string, Set-Cookie
    lists (the value is the cookie string).  FALLBACK rows: valid 0, no entries."""
    import test_emu_parity as tep
    fmt, fields, path, lines = {
        "cookie": (tep.COOKIE_FMT, ["HTTP.COOKIE:request.cookies.*"], "HTTP.COOKIE:request.cookies.*",
                   lambda: tep.cookie_lines(2000, 21)),
        "querystring": (tep.QS_FMT, ["STRING:request.querystring.*"], "STRING:request.querystring.*",
                        lambda: tep.querystring_lines(2000, 22)),
        "setcookie": (tep.SETCOOKIE_FMT, tep.SETCOOKIE_FIELDS[0], "HTTP.SETCOOKIE:response.cookies.*",
                      lambda: tep.setcookie_lines(2000, 32)),
    }[kind]
    lines = lines()
    r, host = check(oracle, kind, fmt, fields, lines, [path])
    c = r.counters
    print(kind, c, "entries", len(host[path]["key_off"]) - 1)
    assert c["ok"] > 1000 and len(host[path]["key_off"]) > 1000
    assert kind == "querystring" or c["fallback"] > 0, c


def test_wave_activity_gpu(oracle):
    """F: batches of 1, 63, 64, 65, 127, 128, 129 lines, every third BAD (its
    timestamp, so the fields include the time)."""
    from test_gpu_parity import paths
    for c in uwc.activity_cases():
        r, _ = check(oracle, c.name, "combined", paths(oracle), c.lines, [REQ, REF], data=c.data)
        assert r.counters["bad"] == len(c.bad)


def test_several_formats_gpu(oracle):
    """Config 5: the rows of a LogFormat that does not deliver the path are
    valid with an empty map."""
    fmt = lpa.SYNTH_FORMATS[lpa.SYNTH_MIXED]
    lines = lpa.synth(lpa.SYNTH_MIXED, 5, 0, 3000).split(b"\n")[:-1]
    fields = [REQ, REF, "HTTP.PATH:request.firstline.uri.path"]
    r, host = check(oracle, "config5", fmt, fields, lines, [REQ, REF])
    valid = host[REF]["valid"]
    per_row = np.diff(host[REF]["entry_off"])
    common = [i for i, l in enumerate(lines) if r.status[i] == lpa.LINE_OK and l.count(b'"') == 2]
    assert len(common) > 300 and all(valid[i] == 1 and per_row[i] == 0 for i in common)
    assert per_row.sum() > 0 and np.diff(host[REQ]["entry_off"]).sum() > 0


WINDOWS = [(0, 0), (1, 63), (1, 64), (3, 65), (64, 129), (-1, 1)]


def _window_of(whole, first, count):
    """rows [first, first + count) of a whole-batch column, rebased to zero"""
    e0, e1 = int(whole["entry_off"][first]), int(whole["entry_off"][first + count])
    out = {"valid": whole["valid"][first:first + count], "entry_off": whole["entry_off"][first:first + count + 1] - e0}
    for off, ch in (("key_off", "key_chars"), ("val_off", "val_chars")):
        b0, b1 = int(whole[off][e0]), int(whole[off][e1])
        out[off] = whole[off][e0:e1 + 1] - b0
        out[ch] = whole[ch][b0:b1]
    return out


def test_row_windows_gpu():
    c = _piece_cases()[-1]
    p = lpa.HttpdLoglineParser("combined", [REQ, REF])
    r = p.parse_batch(c.data)
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    whole = {k: {n: _np(a) for n, a in v.items()} for k, v in r.table_map_device([REQ, REF], decode=False).items()}
    for first, count in WINDOWS:
        first = r.n_lines - 1 if first < 0 else first
        want = {path: _window_of(whole[path], first, count) for path in (REQ, REF)}
        _same_arrays(r.table_map_device([REQ, REF], first, count, decode=False), want, ("device", first, count))
        _same_arrays(r.table_map_from(res, [REQ, REF], first, count, threads=3, decode=False), want,
                     ("host", first, count))


def _raw_call(r, res, path, first, count, caps, on_host):
    """one lp_result_table_map call into buffers of exactly caps = (entries,
    key bytes, value bytes) followed by sentinels; returns (rc, lengths, buffers)"""
    import torch
    n_e, n_k, n_v = caps
    # every byte 0x5A, the int64 arrays' too
    mk = (lambda n, dt: np.full(n * np.dtype(dt).itemsize, 0x5A, dtype=np.uint8).view(dt)) if on_host else (
        lambda n, dt: torch.full((n * np.dtype(dt).itemsize,), 0x5A, dtype=torch.uint8, device="cuda").view(
            {np.uint8: torch.uint8, np.int64: torch.int64}[dt]))
    b = {"valid": mk(count + 8, np.uint8), "entry_off": mk(count + 2, np.int64), "key_off": mk(n_e + 2, np.int64),
         "val_off": mk(n_e + 2, np.int64), "key_chars": mk(n_k + 8, np.uint8), "val_chars": mk(n_v + 8, np.uint8)}
    ptr = (lambda a: a.ctypes.data) if on_host else (lambda a: a.data_ptr())
    col = lpa.LpTableMapCol()
    col.path = path.encode()
    for n in lpa.MAP_ARRAYS:
        setattr(col, n, ptr(b[n]))
    col.entries_cap, col.key_chars_cap, col.val_chars_cap = n_e, n_k, n_v
    rc = lpa.lib().lp_result_table_map(r._p._h, ctypes.byref(res), first, count, ctypes.byref(col), 1, 2)
    return rc, (int(col.entries_len), int(col.key_chars_len), int(col.val_chars_len)), {n: _np(a) for n, a in b.items()}


@pytest.mark.parametrize("on_host", [False, True])
def test_size_protocol_gpu(on_host):
    """lp_result_table's protocol: LP_E_NOMEM with the three exact lengths
    until every capacity suffices; nothing is written past a capacity."""
    c = _piece_cases()[2]
    p = lpa.HttpdLoglineParser("combined", [REQ])
    r = p.parse_batch(c.data)
    hbuf, hres = r.copy_to_host()  # (hres points into hbuf: it stays alive)
    res = hres
    if not on_host:
        res = lpa.LpResult()
        assert lpa.lib().lp_result_view(p._h, ctypes.byref(res)) == lpa.LP_OK
    want = r.table_map_from(hres, [REQ], decode=False)[REQ]
    need = (len(want["key_off"]) - 1, len(want["key_chars"]), len(want["val_chars"]))
    assert min(need) > 64, need
    n = r.n_lines
    rc, got, _b = _raw_call(r, res, REQ, 0, n, (0, 0, 0), on_host)
    assert rc == lpa.LP_E_NOMEM and got == need, (rc, got, need)
    for short in range(3):  # each capacity one short in turn
        caps = tuple(x - (1 if k == short else 0) for k, x in enumerate(need))
        rc, got, b = _raw_call(r, res, REQ, 0, n, caps, on_host)
        assert rc == lpa.LP_E_NOMEM and got == need, (short, rc, got, need)
        for name, used in (("key_off", caps[0] + 1), ("val_off", caps[0] + 1), ("key_chars", caps[1]),
                           ("val_chars", caps[2]), ("valid", n), ("entry_off", n + 1)):
            assert (b[name].view(np.uint8)[used * b[name].itemsize:] == 0x5A).all(), (short, name)
    rc, got, b = _raw_call(r, res, REQ, 0, n, need, on_host)
    assert rc == lpa.LP_OK and got == need
    for name, used in (("valid", n), ("entry_off", n + 1), ("key_off", need[0] + 1), ("val_off", need[0] + 1),
                       ("key_chars", need[1]), ("val_chars", need[2])):
        assert b[name][:used].tobytes() == want[name].tobytes(), name
        assert (b[name].view(np.uint8)[used * b[name].itemsize:] == 0x5A).all(), name  # the sentinel words / bytes


def test_reused_handle_and_buffers_gpu():
    """One handle (two LogFormats) and one set of buffers prefilled with 0xA5:
    batch E, the cookie corpus, E again -- nothing stale is read or left.  The
    reference for each batch is the host replay of that batch on the same
    handle (the handle's active LogFormat is sticky, as the reference's: after
    the cookie batch an E line may be routed otherwise than on a fresh
    handle); the first two batches equal a fresh handle's too."""
    import torch
    import test_emu_parity as tep
    fmt = "combined\n" + tep.COOKIE_FMT
    paths = [REQ, "HTTP.COOKIE:request.cookies.*"]
    big = _piece_cases()[-1]
    cookie = b"".join(l + b"\n" for l in tep.cookie_lines(2000, 21))
    fresh = {}
    for name, data in (("E", big.data), ("cookie", cookie)):
        r = lpa.HttpdLoglineParser(fmt, paths).parse_batch(data)
        fresh[name] = {k: {n: _np(a) for n, a in v.items()} for k, v in r.table_map_device(paths, decode=False).items()}
    # (E has thousands of pieces but eight names: most collapse)
    assert len(fresh["E"][REQ]["key_off"]) > 500 and len(fresh["cookie"][paths[1]]["key_off"]) > 1000
    assert len(fresh["E"][paths[1]]["key_off"]) == 1  # 'combined' rows: valid, no cookies
    p = lpa.HttpdLoglineParser(fmt, paths)
    bufs = None
    for k, (name, data) in enumerate((("E", big.data), ("cookie", cookie), ("E", big.data))):
        r = p.parse_batch(data)
        if bufs is None:
            bufs = r.table_map_buffers(paths, 4096, 1 << 16, 1 << 19, 1 << 19)
            keep = [dict(b) for b in bufs]
        for b in bufs:
            for t in b.values():
                t.view(torch.uint8).fill_(0xA5)
        assert r.n_lines <= 4096
        dev = r.table_map_device(paths, buffers=bufs, decode=False)
        assert all(b[n] is kb[n] for b, kb in zip(bufs, keep) for n in b), "a buffer was too small"
        hbuf, res = r.copy_to_host()  # (res points into hbuf)
        _same_arrays(dev, r.table_map_from(res, paths, threads=4, decode=False), (k, name))
        if k < 2:
            _same_arrays(dev, fresh[name], (k, name, "fresh"))
        assert dev[REQ]["key_off"].numel() > 500


def test_errors_gpu(oracle):
    import remap_corpus as rc
    p = lpa.HttpdLoglineParser("combined", [REQ, "HTTP.PATH:request.firstline.uri.path"])
    r = p.parse_batch(HEAD % (b"/p?a=1", b"-") + b"\n")
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    view = lpa.LpResult()
    assert lpa.lib().lp_result_view(p._h, ctypes.byref(view)) == lpa.LP_OK
    for x, on_host in ((res, True), (view, False)):
        assert _raw_call(r, x, "HTTP.PATH:request.firstline.uri.path", 0, 1, (8, 8, 8), on_host)[0] == lpa.LP_E_INVALID
        assert _raw_call(r, x, "STRING:request.firstline.uri.query.a", 0, 1, (8, 8, 8), on_host)[0] == lpa.LP_E_INVALID
        assert _raw_call(r, x, "STRING:request.referer.query.*", 0, 1, (8, 8, 8), on_host)[0] == lpa.LP_E_MISSING
        assert _raw_call(r, x, REQ, 0, 2, (8, 8, 8), on_host)[0] == lpa.LP_E_INVALID  # past the batch
    # a remapped parameter below the wildcard: the host replay answers
    # (without the corpus' STRING paths two levels down: the oracle's record keys a value by its
    # full path, which does not say whether "url.query.x" is a parameter's name or a nested delivery)
    fields = [f for f in rc.FIELDS if not f.startswith("STRING:" + rc._U + ".")] + [REQ]
    lines = rc.corpus(3, 600)
    p = lpa.HttpdLoglineParser(rc.FORMAT, fields)
    for n, t in rc.REMAPS:
        p.add_type_remapping(n, t)
    r = p.parse_batch(b"".join(l + b"\n" for l in lines))
    with pytest.raises(lpa.FallbackRequired):
        r.table_map_device([REQ])
    hbuf, res = r.copy_to_host()  # (res points into hbuf)
    got = r.table_map_from(res, [REQ])[REQ]
    ref = tmr.oracle_maps(oracle, "remap", rc.FORMAT, fields, lines, [REQ], tuple(rc.REMAPS))
    n_ok = 0
    for i in range(r.n_lines):
        if r.status[i] == lpa.LINE_OK:
            assert got[i] == ref[i][REQ], (i, lines[i], got[i], ref[i][REQ])
            n_ok += 1
        else:
            assert got[i] is None
    assert n_ok > 300
