"""Value edges of the time fields and the typed-table conversions, GPU part:
the corpora of value_edge_corpus.py through the parse kernels and the device
table (table_value.h, table.hip, dict.hip), every column compared with the
corpus' own expectations (datetime / calendar / int / float) exactly --
validity bytes, int64 values, double bit patterns, Arrow offsets and bytes.
No tolerance anywhere.  The only lines left out of a comparison are those
whose local or UTC year is 10000; the test asserts that set (13 of 14 144 in
the date-time layouts) and that the device sends exactly them to FALLBACK.
The CPU part (the corpus pinned against the oracle and the emulation, the
stand-alone program of csrc/lp_value.h) is test_value_edges.py.

Checked by reverting on a scratch copy: without time_fields' year-9999 check
the time tests fail (the 13 lines are OK, TIME.DATE ":000-01-01"); with
decimal_to_double's round-half-even condition flipped test_numbers_gpu fails
on the exact ties ("9007199254740993.0")."""
import functools

import numpy as np
import pytest

import dict_corpus as dc
import logparser_amd as lpa
import value_edge_corpus as vc

pytestmark = pytest.mark.gpu


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _join(lines):
    return b"".join(l + b"\n" for l in lines)


def _arrow(values):
    """a plain Arrow STRING column of bytes | None values"""
    off = np.zeros(len(values) + 1, dtype=np.int64)
    np.cumsum([len(v or b"") for v in values], out=off[1:])
    chars = np.frombuffer(b"".join(v or b"" for v in values), dtype=np.uint8)
    return off, chars, np.array([v is not None for v in values], dtype=np.uint8)


def _by_path(e):
    """a time expectation keyed by path"""
    return None if e is None else {p: e[k] for p, _, k in vc.TIME_FIELDS}


def _table(r, cols, **kw):
    """table_device in calls of at most 24 columns with distinct paths: {(path, type): (values, valid)}"""
    chunks = []
    for c in cols:
        for ch in chunks:
            if len(ch) < 24 and all(x[0] != c[0] for x in ch):
                ch.append(c)
                break
        else:
            chunks.append([c])
    out = {}
    for ch in chunks:
        t = r.table_device(ch, **kw)
        for path, typ in ch:
            out[(path, typ)] = t[path]
    return out


def _check_columns(r, cols, exps, what, **kw):
    """the device columns of the rows whose expectations are exps (None: a row without a record),
    bit for bit"""
    got = _table(r, cols, **kw)
    for path, typ in cols:
        want = [vc.column_expectation(path, typ, e) for e in exps]
        wv = np.array([ok for ok, _ in want], dtype=np.uint8)
        vals, valid = got[(path, typ)]
        valid = _np(valid)
        assert valid.dtype == np.uint8 and valid.shape == wv.shape, (what, path, typ)
        assert valid.tobytes() == wv.tobytes(), (what, path, typ, "valid", int(np.argmax(valid != wv)))
        if typ is str:
            woff, wchars, _ = _arrow([v if ok else None for ok, v in want])
            off, chars = _np(vals[0]), _np(vals[1])
            assert off.dtype == np.int64 and off.tobytes() == woff.tobytes(), \
                (what, path, "offsets", int(np.argmax(off != woff)))
            assert chars.tobytes() == wchars.tobytes(), (what, path, "chars")
        elif typ is int:
            w = np.array([v if ok else 0 for ok, v in want], dtype=np.int64)
            g = np.where(wv.astype(bool), _np(vals), 0)
            assert g.tobytes() == w.tobytes(), (what, path, "long", int(np.argmax(g != w)))
        else:  # doubles by bit pattern
            w = np.array([v if ok else 0.0 for ok, v in want], dtype=np.float64).view(np.uint64)
            g = np.where(wv.astype(bool), _np(vals).view(np.uint64), np.uint64(0))
            assert g.tobytes() == w.tobytes(), (what, path, "double", int(np.argmax(g != w)))


TIME_COLS = [(p, t) for p, t, _ in vc.TIME_FIELDS]


def _check_time(r, layout, at=None, what=None):
    """a parsed batch holding the layout's corpus (line k at row at[k]): the year-10000 lines -- the
    lines without an expectation, that set asserted -- FALLBACK, every other line OK, and every time
    field's device column equal to the expectation"""
    _, lines, exp, none, y10k = vc.time_corpus(layout)
    assert none == y10k and len(none) == (1 if layout == "epoch" else 13)
    at = list(range(len(lines))) if at is None else at
    want = np.full(r.n_lines, lpa.LINE_BAD, dtype=np.uint8)  # (the short lines between them)
    want[at] = lpa.LINE_OK
    want[[at[k] for k in none]] = lpa.LINE_FALLBACK
    assert r.status.tobytes() == want.tobytes(), (what, layout, int(np.argmax(r.status != want)))
    assert r.counters["fallback"] == len(none) and r.counters["ok"] == len(lines) - len(none)
    rows = [None] * r.n_lines
    for k, e in enumerate(exp):
        rows[at[k]] = _by_path(e)
    _check_columns(r, TIME_COLS, rows, (what, layout))


def _oracle_stride(oracle, r, fmt, fields, lines, stride):
    o = oracle.Oracle(fmt, fields)
    n = 0
    for i in range(0, len(lines), stride):
        if int(r.status[i]) == lpa.LINE_OK:
            assert o.parse_raw(lines[i]) == (oracle.OK, r.record_json(i)), (i, lines[i])
            n += 1
    assert n >= len(lines) // stride - 13


# ------------------------------------------------------------------ time
INSTANCES = {
    "fixed_shape": {},                                      # k_parse_chunks' fixed-shape instance
    "generic": {"options": {lpa.OPT_FIXED_SHAPE: 0}},       # its generic instance
    "direct": {"force_direct": True},                       # the HBM / SWAR path
    "deferred": {"options": {lpa.OPT_CHUNK_WAIT: -1}},      # k_parse_deferred
    "overflow": {},                                         # k_parse_ovf_lines: runs of one-byte lines between
}


@pytest.mark.parametrize("instance", list(INSTANCES))
def test_apache_time_instances_gpu(oracle, instance):
    """the Apache layout inside 'combined', every path requested, under each kernel instance that
    inlines the calendar code: each one's columns equal the expectation (so all five agree)"""
    fmt, lines, _, _, _ = vc.time_corpus("apache")
    fields = lpa.get_possible_paths(fmt)
    p = lpa.HttpdLoglineParser(fmt, fields, **INSTANCES[instance])
    batch, at = (lines, None) if instance != "overflow" else vc.interleave_short_lines(lines, 7)
    r = p.parse_batch(_join(batch))
    assert r.n_lines == len(batch)
    if instance == "fixed_shape":
        assert r.diag["fixed_shape"] != 0, r.diag
        _oracle_stride(oracle, r, fmt, fields, lines, 97)
    elif instance == "generic":
        assert r.diag["fixed_shape"] == 0, r.diag
    elif instance == "deferred":
        assert r.diag["deferred_chunks"] > 0, r.diag
    elif instance == "overflow":
        assert r.diag["overflow_waves"] > 0, r.diag
    _check_time(r, "apache", at, instance)


@pytest.mark.parametrize("layout", ["iso", "strf", "epoch"])
def test_time_layouts_gpu(oracle, layout):
    """$time_iso8601, strftime "%F %T %z" and strftime %s (253402300800: past year 9999, FALLBACK)"""
    fmt, lines, _, _, _ = vc.time_corpus(layout)
    fields = [f for f in lpa.get_possible_paths(fmt) if not f.endswith("*")]
    r = lpa.HttpdLoglineParser(fmt, fields).parse_batch(_join(lines))
    assert r.n_lines == len(lines)
    _check_time(r, layout)
    _oracle_stride(oracle, r, fmt, fields, lines, 1 if layout == "epoch" else 97)


# --------------------------------------------------------------- numbers
@functools.lru_cache(None)
def _numbers():
    """the number corpus parsed once for the module: (parser, result, columns)"""
    lines, exp = vc.number_corpus()
    p = lpa.HttpdLoglineParser(vc.NUM_FMT, vc.num_paths())
    r = p.parse_batch(_join(lines))
    assert r.n_lines == len(lines)
    want = [lpa.LINE_BAD if e is None else lpa.LINE_OK for e in exp]
    assert r.status.tolist() == want
    cols = [(f, str) for f in vc.num_paths()]
    cols += [(f, int) for f in vc.num_paths() if (p.get_casts(f) or 0) & lpa.CAST_LONG]
    cols += [(f, float) for f in vc.num_paths() if (p.get_casts(f) or 0) & lpa.CAST_DOUBLE]
    return p, r, cols


def test_numbers_gpu():
    """STRING, LONG and DOUBLE columns (casts permitting) of every path of the number format against
    the Python expectations, and against the host table; no column is host-only"""
    from test_gpu_parity import _device_vs_host_table
    p, r, cols = _numbers()
    _, exp = vc.number_corpus()
    kinds = {t for _, t in cols}
    assert kinds == {str, int, float}
    assert ("PORT:nginxmodule.realip.remote_port", int) in cols  # parse_long's sign branch
    assert any(vc.is_list_item(f) and t is float for f, t in cols)  # decimal_to_double
    _check_columns(r, cols, exp, "numbers")
    _, res = r.copy_to_host()
    assert _device_vs_host_table(r, res, cols) == []


@pytest.mark.parametrize("count", [1, 63, 64, 65, None])
def test_number_windows_gpu(count):
    """table_device(first=k, count=m) with odd firsts: the chars base misaligned, a partial last wave"""
    p, r, cols = _numbers()
    _, exp = vc.number_corpus()
    for first in (1, 67):
        m = r.n_lines - first if count is None else count
        _check_columns(r, cols, exp[first:first + m], ("window", first, m), first=first, count=m)


@pytest.mark.parametrize("which", ["reversed", "strided"])
def test_number_row_lists_gpu(which):
    """the row-list instances of the table kernels: a reversed and a strided device row list"""
    p, r, cols = _numbers()
    _, exp = vc.number_corpus()
    rows = np.arange(r.n_lines - 1, -1, -1) if which == "reversed" else np.arange(3, r.n_lines, 7)
    _check_columns(r, cols, [exp[k] for k in rows], which, rows=_dev(rows))


def _check_dict(r, paths, exps, what, **kw):
    got = r.table_dict_device(paths, **kw)
    for path in paths:
        want = [vc.column_expectation(path, str, e) for e in exps]
        off, chars, valid = _arrow([v if ok else None for ok, v in want])
        widx, woff, wchars = dc.expected_dict(off, chars, valid)
        idx, (doff, dchars), gvalid = got[path]
        assert _np(gvalid).astype(np.uint8).tobytes() == valid.tobytes(), (what, path, "valid")
        assert _np(doff).tobytes() == woff.tobytes(), (what, path, "dict_off")
        assert _np(dchars).tobytes() == wchars.tobytes(), (what, path, "dict_chars")
        assert _np(idx).dtype == np.int32 and _np(idx).tobytes() == widx.tobytes(), (what, path, "index")


def test_dictionary_columns_gpu():
    """table_dict_device: two formatted-long STRING columns (1 to 20 characters, negatives, nulls)
    and TIME.DATE against expected_dict of the expected plain column; a window and a row list too"""
    p, r, _ = _numbers()
    _, exp = vc.number_corpus()
    paths = ["MILLISECONDS:response.server.processing.time", "MICROSECONDS:nginxmodule.upstream.response.time.1.value"]
    _check_dict(r, paths, exp, "numbers")
    _check_dict(r, paths, exp[67:67 + 65], "numbers window", first=67, count=65)
    rows = np.arange(r.n_lines - 1, -1, -3)
    _check_dict(r, paths, [exp[k] for k in rows], "numbers rows", rows=_dev(rows))
    fmt, lines, texp, _, _ = vc.time_corpus("apache")
    date = [f for f, _, k in vc.TIME_FIELDS if k in ("date", "date_utc")]
    rt = lpa.HttpdLoglineParser(fmt, [f for f, _ in TIME_COLS]).parse_batch(_join(lines))
    _check_dict(rt, date, [_by_path(e) for e in texp], "dates")
