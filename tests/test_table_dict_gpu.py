"""Dictionary-encoded STRING columns, GPU part: lp_result_table_dict /
lp_result_table_dict_rows on a device view (dict.hip: the lock-free hash
insert, the representatives' ranks, the indices; the dictionary's values by
table.hip's row-list instances).  Every comparison is bit-exact.  The truth is
the device's own plain STRING column of the same rows (pinned against the host
replay and the oracle by test_gpu_parity / test_row_select_gpu), factorised by
first occurrence in numpy (dict_corpus.expected_dict); the host-copy call must
give arrays identical to the device call's.  The CPU part is test_table_dict.py.

The device-side bound check of a row list is deliberately not exercised here
(as in test_row_select_gpu.py): the host-copy test pins the return code."""
import ctypes
import functools

import numpy as np
import pytest

import dict_corpus as dc
import logparser_amd as lpa
import row_select_corpus as rsc

pytestmark = pytest.mark.gpu

ALL = [dc.UA, dc.PATH, dc.QUERY, dc.STATUS, dc.BYTES, dc.DATE, dc.MONTHNAME, dc.METHOD, dc.REFERER, dc.PARAM_A, dc.PARAM_E]


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


@functools.lru_cache(None)
def _parser(fmt=dc.FMT):
    """one handle per LogFormat for the whole module: every path of the format and the request's query wildcard"""
    return lpa.HttpdLoglineParser(fmt, [f for f in lpa.get_possible_paths(fmt) if not f.endswith("*")] + [dc.REQ])


def _parse(lines, parser=None, statuses=None):
    r = (parser or _parser()).parse_batch(dc.join_lf(lines))
    assert r.n_lines == len(lines)
    assert r.status.tolist() == (statuses if statuses is not None else [lpa.LINE_OK] * len(lines))
    return r


def _view(r):
    v = lpa.LpResult()
    assert lpa.lib().lp_result_view(r._p._h, ctypes.byref(v)) == lpa.LP_OK
    return v


def _same(got, want, what):
    """(index, (dict_off, dict_chars), valid) against expected arrays, bit for bit"""
    (gi, (go, gc), gv), (wi, wo, wc, wv) = got, want
    gi, go, gc, gv = _np(gi), _np(go), _np(gc), _np(gv)
    assert gv.astype(np.uint8).tobytes() == np.asarray(wv, dtype=np.uint8).tobytes(), (what, "valid")
    assert go.dtype == np.int64 and go.tobytes() == wo.tobytes(), (what, "dict_off", go.tolist()[:8], wo.tolist()[:8])
    assert gc.tobytes() == wc.tobytes(), (what, "dict_chars")
    assert gi.dtype == np.int32 and gi.tobytes() == wi.tobytes(), (what, "index")


def _check(r, paths, first=0, count=None, rows=None, res=None, what=None):
    """table_dict_device == expected_dict(the device's plain column) == table_dict_from, per path"""
    kw = {"rows": _dev(rows)} if rows is not None else {"first": first, "count": count}
    plain = r.table_device([(p, str) for p in paths], **kw)
    got = r.table_dict_device(paths, **kw)
    host = None
    if res is not None:
        hkw = {"rows": np.ascontiguousarray(rows, dtype=np.int64)} if rows is not None else {"first": first, "count": count}
        host = r.table_dict_from(res, paths, threads=3, **hkw)
    out = {}
    for p in paths:
        (off, chars), valid = plain[p]
        off, chars, valid = _np(off), _np(chars), _np(valid)
        want = dc.expected_dict(off, chars, valid) + (valid,)
        _same(got[p], want, (what, p, "device"))
        if host is not None:
            _same(host[p], want, (what, p, "host"))
        # decoded: the plain column's strings (bytes: "@line" is not validated UTF-8)
        b = chars.tobytes()
        gi, (go, gc), gv = (_np(got[p][0]), tuple(_np(x) for x in got[p][1]), _np(got[p][2]))
        d = gc.tobytes()
        for k in range(len(valid)):
            if valid[k]:
                assert d[go[gi[k]]:go[gi[k] + 1]] == b[off[k]:off[k + 1]], (what, p, k)
            else:
                assert gi[k] == 0, (what, p, k)
        ents = [d[go[j]:go[j + 1]] for j in range(len(go) - 1)]
        assert len(set(ents)) == len(ents), (what, p, "entries are pairwise distinct")
        out[p] = (gi, go, gc, gv, ents)
    return out


# ------------------------------------------------------------------- 1. sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1500])
def test_sizes_gpu(n):
    """row counts around a wave's 64 and a block's 256 rows, and several blocks;
    all three statuses (a BAD / FALLBACK line's row is null)"""
    ls = rsc.pattern_lines(max(n, 1), "mixed")
    r = _parser().parse_batch(rsc.join_lf([l for l, _ in ls]))
    assert r.status.tolist() == [s for _, s in ls]
    _, res = r.copy_to_host()
    paths = [dc.UA, dc.PATH, dc.STATUS, dc.DATE, dc.REFERER]
    out = _check(r, paths, 0, n, res=res, what=n)
    if n == 0:
        assert all(len(v[4]) == 0 and v[1].tolist() == [0] for v in out.values())
    if n >= 63:
        assert len(out[dc.UA][4]) == 1 and len(out[dc.REFERER][4]) > n // 3  # (two OK lines in three have a referer)


# ------------------------------------------------------------ 2. value shapes
def test_value_shapes_gpu():
    """one handle with every path: pointer values, a raw query string with its
    '&', longs rendered as text, formatted values, "@line" over a row list, a
    4 KB user agent, a column whose every value is "" """
    big = b"B" * 4096
    lines = [dc.line(k, ua=big if k in (3, 77) else b"ua-%d" % (k % 9)) for k in range(300)]
    r = _parse(lines)
    _, res = r.copy_to_host()
    out = _check(r, ALL, res=res, what="shapes")
    assert big in out[dc.UA][4] and len(out[dc.UA][4]) == 10
    assert all(e.startswith(b"&e=&a=") for e in out[dc.QUERY][4]) and len(out[dc.QUERY][4]) == 5
    assert sorted(out[dc.STATUS][4]) == [b"200", b"301", b"404"]
    assert b"0" in out[dc.BYTES][4] and b"5000" in out[dc.BYTES][4]  # "-" -> 0
    assert b"2026-10-11" in out[dc.DATE][4] and set(out[dc.MONTHNAME][4]) == {
        b"January", b"February", b"March", b"October", b"December"}
    assert out[dc.PARAM_E][4] == [b""] and out[dc.PARAM_E][3].all()  # "" is a value
    assert not out[dc.REFERER][3].any() and out[dc.REFERER][4] == []  # "-": null, no entry
    rows = np.array([7, 3, 7, 299, 3, 0], dtype=np.int64)
    ln = _check(r, ["@line", dc.UA], rows=rows, res=res, what="@line")
    assert ln["@line"][4] == [lines[7], lines[3], lines[299], lines[0]] and ln["@line"][0].tolist() == [0, 1, 0, 2, 1, 3]
    assert _check(r, ["@line"], 10, 20, res=res, what="@line window")["@line"][4] == lines[10:30]


# ------------------------------------------------------------- 3. cardinality
def test_cardinality_gpu():
    same = _check(_parse([dc.line(k, ua=b"one", path=b"/x", a=b"1", status=200, size=b"5") for k in range(700)]),
                  ALL, what="same")
    assert all(len(v[4]) <= 1 for p, v in same.items() if p not in (dc.DATE, dc.MONTHNAME))
    n = 4099  # every row distinct: the table at its load limit
    r = _parse([dc.line(k, ua=b"agent %d" % k, path=b"/d/%d" % (k * 7919), a=b"%x" % k) for k in range(n)])
    _, res = r.copy_to_host()
    out = _check(r, [dc.UA, dc.PATH, dc.PARAM_A, dc.QUERY], res=res, what="distinct")
    assert all(len(v[4]) == n and v[0].tolist() == list(range(n)) for v in out.values())
    # values equal in their first 64 bytes and different after; values equal except in length
    pre = b"P" * 64
    lines = [dc.line(k, ua=pre + b"%d" % (k % 11), a=b"a" * (k % 23)) for k in range(400)]
    out = _check(_parse(lines), [dc.UA, dc.PARAM_A, dc.QUERY], what="prefixes")
    assert len(out[dc.UA][4]) == 11 and out[dc.PARAM_A][4] == [b"a" * k for k in range(23)]


def test_no_valid_row_gpu():
    r = _parse([rsc.bad_line(k) for k in range(130)], statuses=[lpa.LINE_BAD] * 130)
    _, res = r.copy_to_host()
    out = _check(r, [dc.UA, dc.STATUS, dc.DATE], res=res, what="all bad")
    assert all(v[4] == [] and v[1].tolist() == [0] and not v[0].any() and not v[3].any() for v in out.values())


# -------------------------------------------------------------- 4. collisions
def test_collisions_gpu():
    """about 300 distinct values with the hash narrowed to 1, 2 and 8 bits:
    the probe and byte-compare paths; the result does not depend on it"""
    p = lpa.HttpdLoglineParser(dc.FMT, [dc.UA, dc.PARAM_A, dc.STATUS, dc.BYTES, dc.DATE])
    lines = [dc.line(k, ua=b"agent/%d" % (k * 31 % 307), a=b"%d" % (k % 301)) for k in range(900)]
    r = _parse(lines, parser=p)
    paths = [dc.UA, dc.PARAM_A, dc.STATUS, dc.BYTES, dc.DATE]
    L = lpa.lib()
    try:
        base = _check(r, paths, what="bits 0")
        assert len(base[dc.UA][4]) == 307 and len(base[dc.PARAM_A][4]) == 301
        for bits in (1, 2, 8):
            assert L.lp_set_option(p._h, lpa.OPT_DICT_HASH_BITS, bits) == lpa.LP_OK
            got = _check(r, paths, what="bits %d" % bits)
            for path in paths:
                for a, b in zip(got[path][:4], base[path][:4]):
                    assert a.tobytes() == b.tobytes(), (bits, path)
    finally:
        L.lp_set_option(p._h, lpa.OPT_DICT_HASH_BITS, 0)
    assert L.lp_set_option(p._h, lpa.OPT_DICT_HASH_BITS, 33) == lpa.LP_E_INVALID
    assert L.lp_set_option(p._h, lpa.OPT_DICT_HASH_BITS, -1) == lpa.LP_E_INVALID


# ------------------------------------------------------- 5. row lists, windows
def test_row_lists_and_windows_gpu():
    """ascending (select_device), descending, with repeats, empty: the order of
    the entries follows the row index k; a window equals the row list of its lines"""
    ls = rsc.pattern_lines(700, "mixed")
    r = _parser().parse_batch(rsc.join_lf([l for l, _ in ls]))
    assert r.status.tolist() == [s for _, s in ls]
    _, res = r.copy_to_host()
    ok = _np(r.select_device(lpa.SEL_OK))
    assert len(ok) > 300
    paths = [dc.REFERER, dc.PATH, dc.DATE, "@line"]
    lists = {"ascending": ok, "descending": ok[::-1], "repeats": np.repeat(ok[:90], 3)[5:], "empty": ok[:0],
             "every line backwards": np.arange(700, dtype=np.int64)[::-1]}
    outs = {name: _check(r, paths, rows=np.ascontiguousarray(rows), res=res, what=name) for name, rows in lists.items()}
    asc, desc = outs["ascending"][dc.REFERER][4], outs["descending"][dc.REFERER][4]
    assert len(asc) > 100 and asc == desc[::-1]  # (every referer of the corpus is distinct or null)
    assert outs["empty"][dc.PATH][4] == [] and outs["empty"]["@line"][1].tolist() == [0]
    for first, count in ((1, 64), (63, 130), (256, 444), (699, 1), (700, 0)):
        w = _check(r, paths, first, count, res=res, what=("window", first, count))
        g = _check(r, paths, rows=np.arange(first, first + count, dtype=np.int64), what=("as rows", first, count))
        for p in paths:
            for a, b in zip(w[p][:4], g[p][:4]):
                assert a.tobytes() == b.tobytes(), (first, count, p)


# ------------------------------------------------------- 6. several LogFormats
def test_several_logformats_gpu():
    """combined and common lines interleaved: a path both formats deliver, and
    one only combined delivers (null in a common line's row)"""
    p = _parser("combined\ncommon")
    lines = [dc.common_line(k) if k % 3 == 1 else dc.line(k, ua=b"ua%d" % (k % 4)) for k in range(333)]
    r = _parse(lines, parser=p)
    _, res = r.copy_to_host()
    out = _check(r, dc.COMMON_FIELDS + [dc.UA, dc.DATE], res=res, what="two formats")
    assert out[dc.STATUS][3].all() and out[dc.BYTES][3].all() and sorted(out[dc.STATUS][4]) == [b"200", b"301", b"404"]
    assert out[dc.UA][3].tolist() == [0 if k % 3 == 1 else 1 for k in range(333)] and len(out[dc.UA][4]) == 4
    rows = np.arange(333, dtype=np.int64)[::-2]
    _check(r, [dc.STATUS, dc.UA], rows=np.ascontiguousarray(rows), res=res, what="two formats, rows")


# ------------------------------------------------------------ 7. size protocol
def _raw(r, res, path, on_host, n, dict_cap, chars_cap, rows=None):
    """one raw call into guarded buffers filled with 0x5A: (rc, dict_len, dict_chars_len, {name: numpy bytes})"""
    import torch
    mk = (lambda nb: np.full(nb, 0x5A, dtype=np.uint8)) if on_host else (
        lambda nb: torch.full((nb,), 0x5A, dtype=torch.uint8, device="cuda"))
    ptr = (lambda a: a.ctypes.data) if on_host else (lambda a: a.data_ptr())
    b = {"valid": mk(n + 8), "index": mk(4 * n + 8), "dict_off": mk(8 * (dict_cap + 1) + 8), "dict_chars": mk(chars_cap + 8)}
    col = lpa.LpTableDictCol()
    col.path = path.encode()
    col.valid, col.index, col.dict_off, col.dict_chars = (ptr(b[k]) for k in ("valid", "index", "dict_off", "dict_chars"))
    col.dict_cap, col.dict_chars_cap = dict_cap, chars_cap
    L = lpa.lib()
    if rows is None:
        rc = L.lp_result_table_dict(r._p._h, ctypes.byref(res), 0, n, ctypes.byref(col), 1, 2)
    else:
        rc = L.lp_result_table_dict_rows(r._p._h, ctypes.byref(res), rows, n, ctypes.byref(col), 1, 2)
    return rc, int(col.dict_len), int(col.dict_chars_len), {k: _np(v) for k, v in b.items()}


@pytest.mark.parametrize("on_host", [False, True])
def test_size_protocol_gpu(on_host):
    lines = [dc.line(k, ua=b"agent-%d" % (k % 37)) for k in range(500)]
    r = _parse(lines)
    hbuf, hres = r.copy_to_host()  # (hres points into hbuf)
    res = hres if on_host else _view(r)
    (off, chars), valid = r.table_device([(dc.UA, str)])[dc.UA]
    wi, wo, wc = dc.expected_dict(_np(off), _np(chars), _np(valid))
    need = (len(wo) - 1, len(wc))
    assert need[0] == 37 and need[1] > 200
    for caps in ((need[0] - 1, need[1]), (need[0], need[1] - 1), (0, need[1]), (need[0], 0), (0, 0)):
        rc, dl, cl, b = _raw(r, res, dc.UA, on_host, 500, *caps)
        assert rc == lpa.LP_E_NOMEM and (dl, cl) == need, (caps, rc, dl, cl, need)
        assert (b["dict_off"][8 * (caps[0] + 1):] == 0x5A).all() and (b["dict_chars"][caps[1]:] == 0x5A).all(), caps
        assert (b["valid"][500:] == 0x5A).all() and (b["index"][2000:] == 0x5A).all(), caps
    rc, dl, cl, b = _raw(r, res, dc.UA, on_host, 500, *need)  # the repeat call
    assert rc == lpa.LP_OK and (dl, cl) == need
    assert b["valid"][:500].tobytes() == _np(valid).tobytes() and (b["valid"][500:] == 0x5A).all()
    assert b["index"][:2000].tobytes() == wi.tobytes() and (b["index"][2000:] == 0x5A).all()
    assert b["dict_off"][:8 * (need[0] + 1)].tobytes() == wo.tobytes() and (b["dict_off"][8 * (need[0] + 1):] == 0x5A).all()
    assert b["dict_chars"][:need[1]].tobytes() == wc.tobytes() and (b["dict_chars"][need[1]:] == 0x5A).all()


# -------------------------------------------------------------------- 8. reuse
def test_reuse_gpu():
    """a large call, then a small one on the same handle and buffers (stale
    slots of the first would show); two handles interleaved"""
    import torch
    p = lpa.HttpdLoglineParser(dc.FMT, [dc.UA, dc.PATH])
    q = lpa.HttpdLoglineParser(dc.FMT, [dc.UA, dc.PATH])
    big = _parse([dc.line(k, ua=b"A%d" % (k % 501), path=b"/%d" % k) for k in range(3000)], parser=p)
    bufs = big.table_dict_buffers([dc.UA, dc.PATH], count=3000, dict_cap=3000, dict_chars_cap=1 << 16)
    keep = [list(b) for b in bufs]
    first = big.table_dict_device([dc.UA, dc.PATH], buffers=bufs)
    assert len(first[dc.UA][1][0]) == 502 and len(first[dc.PATH][1][0]) == 3001
    other = _parse([dc.line(k, ua=b"Q%d" % (k % 3)) for k in range(200)], parser=q)
    small = _parse([dc.line(k, ua=b"A%d" % (500 - k % 5), path=b"/%d" % (2999 - k % 2)) for k in range(70)], parser=p)
    for b in bufs:
        for t in b:
            t.view(torch.uint8).fill_(0xA5)
    for r, paths in ((other, [dc.UA]), (small, [dc.UA, dc.PATH]), (other, [dc.PATH, dc.UA])):
        plain = r.table_device([(x, str) for x in paths])
        got = r.table_dict_device(paths, buffers=bufs[:len(paths)])
        assert all(x is y for b, kb in zip(bufs, keep) for x, y in zip(b, kb)), "a buffer was too small"
        for x in paths:
            (off, chars), valid = plain[x]
            _same(got[x], dc.expected_dict(_np(off), _np(chars), _np(valid)) + (_np(valid),), ("reuse", r.n_lines, x))
    assert (_np(bufs[0][1][200:].view(torch.uint8)) == 0xA5).all()  # nothing written past the later calls' rows


# ----------------------------------------------------------- 9. several columns
def test_several_columns_gpu():
    r = _parse([dc.line(k, ua=b"u%d" % (k % 13)) for k in range(777)])
    together = r.table_dict_device(ALL)
    for p in ALL:
        alone = r.table_dict_device([p])[p]
        _same(together[p], (_np(alone[0]), _np(alone[1][0]), _np(alone[1][1]), _np(alone[2])), ("alone", p))
    t = r.table_dict_timing()
    assert set(t) == {"values", "insert", "index", "dict"} and all(v > 0 for v in t.values())


# ------------------------------------------------------------------ 10. errors
def test_errors_gpu():
    p = lpa.HttpdLoglineParser(dc.FMT, [dc.UA, dc.REQ, "TIME.EPOCH:request.receive.time.epoch"])
    r = _parse([dc.line(k) for k in range(80)], parser=p)
    hbuf, hres = r.copy_to_host()  # (hres points into hbuf)
    view = _view(r)
    L = lpa.lib()

    def untouched(b):
        return all((a == 0x5A).all() for a in b.values())
    # host copy: an index outside [0, n_lines) is refused before anything is written
    for bad in (-1, 80, 1 << 40):
        rows = np.array([3, 0, bad, 5], dtype=np.int64)
        rc, _dl, _cl, b = _raw(r, hres, dc.UA, True, 4, 8, 256, rows=rows.ctypes.data)
        assert rc == lpa.LP_E_INVALID and untouched(b), bad
    rows = np.array([3, 0, 79, 5], dtype=np.int64)
    rc, dl, _cl, b = _raw(r, hres, dc.UA, True, 4, 8, 256, rows=rows.ctypes.data)
    assert rc == lpa.LP_OK and dl == 1
    # a device view takes device memory only: host rows and host arrays are refused, never dereferenced
    rc, _dl, _cl, b = _raw(r, view, dc.UA, False, 4, 8, 256, rows=rows.ctypes.data)
    assert rc == lpa.LP_E_INVALID and untouched(b)
    rc, _dl, _cl, b = _raw(r, view, dc.UA, True, 80, 8, 256)  # host arrays on the device view
    assert rc == lpa.LP_E_INVALID and untouched(b)
    with pytest.raises(ValueError):
        r.table_dict_device([dc.UA], rows=rows)  # (the mirror refuses a numpy array there too)
    with pytest.raises(ValueError):
        r.table_dict_device([dc.UA], rows=_dev(rows), first=1)
    # paths: not delivered; a pseudo-column that is not "@line" (a LONG)
    for on_host, res in ((False, view), (True, hres)):
        for path, want in (("STRING:request.nothing", lpa.LP_E_MISSING), ("@nothing", lpa.LP_E_MISSING),
                           ("@offset", lpa.LP_E_INVALID), ("@status", lpa.LP_E_INVALID)):
            rc, _dl, _cl, b = _raw(r, res, path, on_host, 80, 8, 256)
            assert rc == want and untouched(b), (on_host, path, rc)
        assert _raw(r, res, dc.UA, on_host, 81, 8, 256)[0] == lpa.LP_E_INVALID  # past the batch
        col = lpa.LpTableDictCol()
        assert L.lp_result_table_dict(p._h, ctypes.byref(res), 0, (1 << 31), ctypes.byref(col), 1, 1) == lpa.LP_E_INVALID
        assert L.lp_result_table_dict_rows(p._h, ctypes.byref(res), None, 3, ctypes.byref(col), 1, 1) == lpa.LP_E_INVALID
    # more columns than the device table takes
    import torch
    many = 33
    cols = (lpa.LpTableDictCol * many)()
    keep = []
    for c in cols:
        t = [torch.zeros(80, dtype=torch.uint8, device="cuda"), torch.zeros(80, dtype=torch.int32, device="cuda"),
             torch.zeros(9, dtype=torch.int64, device="cuda"), torch.zeros(256, dtype=torch.uint8, device="cuda")]
        keep.append(t)
        c.path = dc.UA.encode()
        c.valid, c.index, c.dict_off, c.dict_chars = (x.data_ptr() for x in t)
        c.dict_cap, c.dict_chars_cap = 8, 256
    assert L.lp_result_table_dict(p._h, ctypes.byref(view), 0, 80, cols, many, 0) == lpa.LP_E_INVALID
    assert L.lp_result_table_dict(p._h, ctypes.byref(view), 0, 80, cols, 32, 0) == lpa.LP_OK
    # a path the device table refuses (a remapped token dissected again: the host replay answers);
    # every STRING path of the handle is either built or refused with nothing written
    import remap_corpus as rc
    q = lpa.HttpdLoglineParser(rc.FORMAT, rc.FIELDS)
    for n, t in rc.REMAPS:
        q.add_type_remapping(n, t)
    r2 = q.parse_batch(dc.join_lf(rc.corpus(3, 40)))
    _, res2 = r2.copy_to_host()
    seen = {}
    for f in rc.FIELDS:
        if f.endswith("*") or not lpa.lib().lp_casts(q._h, f.encode()) & lpa.CAST_STRING:
            continue
        rc_, _dl, _cl, b = _raw(r2, _view(r2), f, False, 40, 64, 1 << 14)
        seen.setdefault(rc_, f)
        assert rc_ in (lpa.LP_OK, lpa.LP_E_UNSUPPORTED), (f, rc_)
        if rc_ == lpa.LP_E_UNSUPPORTED:
            assert untouched(b), f
            with pytest.raises(lpa.FallbackRequired):
                r2.table_dict_device([f])
            r2.table_dict_from(res2, [f])  # the host copy builds it
        else:
            _check(r2, [f], res=res2, what=("remap", f))
    assert set(seen) == {lpa.LP_OK, lpa.LP_E_UNSUPPORTED}, seen
    # a view of an older batch
    r3 = _parse([dc.line(k) for k in range(33)], parser=p)
    rc, _dl, _cl, b = _raw(r3, view, dc.UA, False, 33, 8, 256)
    assert rc in (lpa.LP_E_STATE, lpa.LP_E_INVALID) and untouched(b)
