"""The GeoIP dissectors on the device: k_geoip_lines (geoip.hip) and the
table's TC_GEOIP gather, on the synthetic databases and the corpus of
geoip_corpus.py.  Two handles on the same input: A is today's program (the
same format without GeoIP), B adds the GeoIP outputs.  A must be unchanged
and never FALLBACK on the planted lines; B's statuses differ from A's exactly
where the independent restatement (geoip_ref.py) leaves the line to the
reference, and every new column equals the expectation exactly -- values,
validity, offsets and bytes, from the device view, the host copy and the emit
stream.  The CPU part is test_geoip.py."""
import functools
import os
import tempfile

import numpy as np
import pytest

import geoip_corpus as gc
import geoip_ref as gr
import logparser_amd as lpa

pytestmark = pytest.mark.gpu

PREFIX = "connection.client.host."
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geoip")
HOST = "IP:connection.client.host"


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def fields_of(cls, prefix=PREFIX):
    return ["%s:%s%s" % (n.split(":")[0], prefix, n.split(":")[1]) for n, _, _ in gr.CLASSES[cls]]


@functools.lru_cache(None)
def _tmp():
    return tempfile.mkdtemp(prefix="geoip_gpu_")


@functools.lru_cache(None)
def _db(name):
    path, data, _ = gc.write_db(_tmp(), name)
    return path, gr.Reader(data)


def _parser(fields, dissectors, fmt=gc.LOGFORMAT, remaps=()):
    p = lpa.HttpdLoglineParser(fmt, list(fields))
    for name, settings in dissectors:
        p.add_dissector(name, settings)
    for path, typ in remaps:
        p.add_type_remapping(path, typ)
    return p


@functools.lru_cache(None)
def _baseline():
    lines = gc.corpus()
    pa = _parser([HOST], [])
    ra = pa.parse_batch(gc.data_of(lines))
    assert pa.device_program_ok, pa.unsupported_reason
    return lines, pa, ra


@functools.lru_cache(None)
def _city(name):
    """the corpus through handle B of database `name`: (parser, result, expectation per line -- None: not OK)"""
    lines, _, ra = _baseline()
    path, rd = _db(name)
    pb = _parser([HOST] + fields_of("GeoIPCityDissector"), [("GeoIPCityDissector", path)])
    rb = pb.parse_batch(gc.data_of(lines))
    assert pb.device_program_ok, pb.unsupported_reason
    exp = []
    for k, (_, host) in enumerate(lines):
        if host is None or ra.status[k] != lpa.LINE_OK:
            exp.append(None)
        else:
            exp.append(gr.dissect(rd, "GeoIPCityDissector", None if host == "-" else host))
    return pb, rb, exp


def _expected_column(exp, name, typ, prefix=""):
    """(valid, values) of output `name` ("TYPE:name" of geoip_ref): text, ints or floats"""
    vals = []
    for e in exp:
        v = None if e is None else e.get(name)
        if v is not None:
            v = str(v) if typ is str else int(v) if typ is int else float(v)
        vals.append(v)
    return np.array([v is not None for v in vals], dtype=bool), vals


def _same_string(got, valid, vals, what):
    (off, chars), ok = got
    off, chars, ok = _np(off).astype(np.int64), _np(chars), _np(ok).astype(bool)
    assert ok.tolist() == valid.tolist(), (what, "valid")
    enc = [v.encode() if v is not None else b"" for v in vals]
    want_off = np.concatenate([[0], np.cumsum([len(b) for b in enc])]).astype(np.int64)
    assert off.tolist() == want_off.tolist(), (what, "offsets")
    assert chars.tobytes()[:want_off[-1]] == b"".join(enc), (what, "bytes")


def _same_number(got, valid, vals, what):
    x, ok = got
    x, ok = _np(x), _np(ok).astype(bool)
    assert ok.tolist() == valid.tolist(), (what, "valid")
    assert [x[k].item() for k in range(len(vals)) if valid[k]] == [v for v in vals if v is not None], (what, "values")


def _path(name, prefix=PREFIX):
    return "%s:%s%s" % (name.split(":")[0], prefix, name.split(":")[1])


def test_handle_a_is_unchanged_gpu():
    lines, pa, ra = _baseline()
    want = [lpa.LINE_OK if h is not None else None for _, h in lines]
    got = ra.status.tolist()
    assert all(w is None or g == w for g, w in zip(got, want))  # never FALLBACK on a planted line
    other = {got[k] for k, w in enumerate(want) if w is None}
    assert other == {lpa.LINE_BAD, lpa.LINE_FALLBACK}
    (off, chars), valid = ra.table_device([(HOST, str)])[HOST]
    off, chars = _np(off), _np(chars).tobytes()
    for k, (_, h) in enumerate(lines):
        if h is not None:
            assert (chars[off[k]:off[k + 1]].decode() if _np(valid)[k] else "-") == h


@pytest.mark.parametrize("name", sorted(gc.CITY_DBS))
def test_status_rule_and_columns_gpu(name):
    """FALLBACK exactly on the planted lines; every new column from the device view and the host copy"""
    lines, _, ra = _baseline()
    pb, rb, exp = _city(name)
    n = len(lines)
    planted = {k for k, e in enumerate(exp) if e is None and ra.status[k] == lpa.LINE_OK}
    want = [lpa.LINE_FALLBACK if k in planted else int(ra.status[k]) for k in range(n)]
    assert rb.status.tolist() == want
    assert rb.counters == {"lines": n, "ok": want.count(lpa.LINE_OK), "bad": want.count(lpa.LINE_BAD),
                           "fallback": want.count(lpa.LINE_FALLBACK)}
    assert {lines[k][1] for k in planted} >= set(gc.UNDECIDED_HOSTS)
    exp_ok = [e if k not in planted else None for k, e in enumerate(exp)]
    outs = [(nm, kind) for nm, kind, _ in gr.CITY]
    dev_s = rb.table_device([(_path(nm), str) for nm, _ in outs])
    nums = [(nm, int if kind.startswith("L") else float) for nm, kind in outs if kind != "S"]
    dev_n = rb.table_device([(_path(nm), t) for nm, t in nums])
    hbuf, res = rb.copy_to_host()  # (hbuf: the copy the result points into)
    host_s = rb.table_from(res, [(_path(nm), str) for nm, _ in outs], decode=False)
    host_n = rb.table_from(res, [(_path(nm), t) for nm, t in nums])
    for nm, _ in outs:
        valid, vals = _expected_column(exp_ok, nm, str)
        _same_string(dev_s[_path(nm)], valid, vals, (nm, "device"))
        _same_string(host_s[_path(nm)], valid, vals, (nm, "host"))
    for nm, t in nums:
        valid, vals = _expected_column(exp_ok, nm, t)
        _same_number(dev_n[_path(nm)], valid, vals, (nm, "device"))
        _same_number(host_n[_path(nm)], valid, vals, (nm, "host"))
    # the geo column itself: from the view's copy, 0 exactly where nothing is delivered
    cols = rb.columns(res)
    geo = cols[("geo", 0)]
    for k, e in enumerate(exp_ok):
        if e is not None:
            assert (geo[k] != 0) == bool(e), k


def test_emit_stream_gpu():
    """lp_result_emit: the outputs in the reference's delivery order, nulls as nulls"""
    lines, _, ra = _baseline()
    pb, rb, exp = _city("v6_28")
    hbuf, res = rb.copy_to_host()  # (hbuf: the copy the result points into)
    names = [nm for nm, _, _ in gr.CITY]
    for i, e in enumerate(exp):
        if e is None:
            continue
        got = [(b, t, n, v) for b, t, n, v in rb.emissions_from(res, i) if b == "connection.client.host" and n]
        want = [("connection.client.host", nm.split(":")[0], nm.split(":")[1], e[nm]) for nm in names if nm in e]
        assert got == want, (i, lines[i][1])
        rec = rb.record(i)
        for nm in names:
            v = rec.get(_path(nm), [])
            assert ([x["l"] if isinstance(x, dict) else x for x in v] or [None])[-1] == e.get(nm), (i, nm)


def test_rows_dict_and_arrow_gpu():
    """a row-list table over the OK rows, a dictionary column of country.name and one Arrow batch"""
    import pyarrow as pa
    lines, _, ra = _baseline()
    pb, rb, exp = _city("v6_28")
    ok = [i for i in range(len(lines)) if rb.status[i] == lpa.LINE_OK]
    rows = rb.select_device(lpa.SEL_OK)
    assert _np(rows).tolist() == ok
    exp_f = [e if rb.status[i] == lpa.LINE_OK else None for i, e in enumerate(exp)]
    exp_ok = [exp_f[i] for i in ok]
    fs = ["STRING:city.name", "NUMBER:city.geonameid", "STRING:location.latitude"]
    t = rb.table_device([(_path(f), str) for f in fs], rows=rows)
    for f in fs:
        valid, vals = _expected_column(exp_ok, f, str)
        _same_string(t[_path(f)], valid, vals, (f, "rows"))
    cn = _path("STRING:country.name")
    valid, vals = _expected_column(exp_f, "STRING:country.name", str)
    for kw, want_valid, want_vals in (({}, valid, vals), ({"rows": rows}, valid[ok], [vals[i] for i in ok])):
        index, (doff, dchars), dvalid = rb.table_dict_device([cn], **kw)[cn]
        got = lpa.strings_from_dict(_np(dvalid), _np(index), _np(doff), _np(dchars))
        assert [g if want_valid[k] else None for k, g in enumerate(got)] == want_vals
        assert _np(dvalid).astype(bool).tolist() == want_valid.tolist()
        assert len(_np(doff)) - 1 == len({v for v in want_vals if v is not None})
    cols = [(cn, "dict", "country"), (_path("STRING:city.name"), str, "city"),
            (_path("NUMBER:city.geonameid"), int, "geoname"), (_path("STRING:location.latitude"), float, "lat"),
            (_path("BOOLEAN:country.isineuropeanunion"), int, "eu")]
    ex = rb.to_arrow_device(cols)
    try:
        batch = ex.to_host()
    finally:
        ex.release()
    assert isinstance(batch, pa.RecordBatch) and batch.num_rows == len(lines)
    batch.validate(full=True)
    for (path, typ, name), out in zip(cols, ["STRING:country.name", "STRING:city.name", "NUMBER:city.geonameid",
                                             "STRING:location.latitude", "BOOLEAN:country.isineuropeanunion"]):
        _, want = _expected_column(exp_f, out, str if typ in (str, "dict") else typ)
        assert batch.column(batch.schema.get_field_index(name)).to_pylist() == want, name


def test_wave_edges_gpu():
    lines, _, _ = _baseline()
    path, rd = _db("v6_28")
    f = [_path("STRING:city.name"), _path("NUMBER:location.accuracyradius")]
    pb = _parser(f, [("GeoIPCityDissector", path)])
    pa = _parser([HOST], [])
    for n in (1, 63, 64, 65, 129):
        sub = lines[:n]
        ra, rb = pa.parse_batch(gc.data_of(sub)), pb.parse_batch(gc.data_of(sub))
        exp = [None if h is None or ra.status[k] != lpa.LINE_OK else gr.dissect(rd, "GeoIPCityDissector", None if h == "-" else h)
               for k, (_, h) in enumerate(sub)]
        want = [lpa.LINE_FALLBACK if e is None and ra.status[k] == lpa.LINE_OK else int(ra.status[k]) for k, e in enumerate(exp)]
        assert rb.status.tolist() == want, n
        assert rb.counters["fallback"] == want.count(lpa.LINE_FALLBACK) and rb.counters["lines"] == n
        exp_ok = [e if want[k] == lpa.LINE_OK else None for k, e in enumerate(exp)]
        t = rb.table_device([(f[0], str), (f[1], int)])
        valid, vals = _expected_column(exp_ok, "STRING:city.name", str)
        _same_string(t[f[0]], valid, vals, (n, "city"))
        valid, vals = _expected_column(exp_ok, "NUMBER:location.accuracyradius", int)
        _same_number(t[f[1]], valid, vals, (n, "radius"))


def test_two_databases_one_handle_gpu():
    """City and ASN on the same token: two stages, two trees"""
    lines, _, ra = _baseline()
    (cpath, crd), (apath, ard) = _db("v6_28"), _db("asn")
    sub = lines[:300]
    f = [_path("STRING:city.name"), _path("ASN:asn.number"), _path("STRING:asn.organization")]
    p = _parser(f, [("GeoIPCityDissector", cpath), ("nl.basjes.parse.httpdlog.dissectors.geoip.GeoIPASNDissector", apath)])
    r = p.parse_batch(gc.data_of(sub))
    assert p.device_program_ok, p.unsupported_reason
    exp = []
    for k, (_, h) in enumerate(sub):
        if h is None or ra.status[k] != lpa.LINE_OK:
            exp.append(None)
            continue
        c = gr.dissect(crd, "GeoIPCityDissector", None if h == "-" else h)
        a = gr.dissect(ard, "GeoIPASNDissector", None if h == "-" else h)
        exp.append(None if c is None else dict(c, **a))
    assert r.status.tolist() == [lpa.LINE_FALLBACK if e is None and ra.status[k] == lpa.LINE_OK else int(ra.status[k])
                                 for k, e in enumerate(exp)]
    t = r.table_device([(f[0], str), (f[1], int), (f[2], str)])
    for path, out, typ, same in ((f[0], "STRING:city.name", str, _same_string), (f[1], "ASN:asn.number", int, _same_number),
                                 (f[2], "STRING:asn.organization", str, _same_string)):
        valid, vals = _expected_column(exp, out, typ)
        assert valid.any()
        same(t[path], valid, vals, out)


def test_two_formats_one_with_the_stage_gpu():
    path, rd = _db("v6_28")
    city = "STRING:connection.client.host.city.name"
    p = _parser([city, "STRING:connection.client.user"], [("GeoIPCityDissector", path)], fmt='%h %l %u\n%u "%{Referer}i"')
    data = b'80.100.1.2 - alice\nbob "http://x/"\nlocalhost - carol\ndave "-"\n1::7 - erin\n' * 13
    r = p.parse_batch(data)
    assert p.device_program_ok, p.unsupported_reason
    assert r.status.tolist() == [lpa.LINE_OK, lpa.LINE_OK, lpa.LINE_FALLBACK, lpa.LINE_OK, lpa.LINE_OK] * 13
    assert r.counters == {"lines": 65, "ok": 52, "bad": 0, "fallback": 13}
    want = [gr.dissect(rd, "GeoIPCityDissector", "80.100.1.2")["STRING:city.name"], None, None, None,
            gr.dissect(rd, "GeoIPCityDissector", "1::7")["STRING:city.name"]] * 13
    _same_string(r.table_device([(city, str)])[city], np.array([v is not None for v in want]), want, "city")


def test_golden_fixtures_and_python_mirror_gpu():
    """the reference's own databases through the public interface: add_dissector, casts, setters, errors"""
    city, asn = os.path.join(GOLD, "GeoIP2-City-Test.mmdb"), os.path.join(GOLD, "GeoLite2-ASN-Test.mmdb")
    with_d = set(lpa.get_possible_paths("%h", dissectors=[("GeoIPCityDissector", city)]))
    assert "STRING:connection.client.host.country.name" in with_d - set(lpa.get_possible_paths("%h"))
    with pytest.raises(lpa.InvalidDissectorException):
        lpa.get_possible_paths("%h", dissectors=[("GeoIPCityDissector", "Does not exist")])
    with pytest.raises(lpa.InvalidDissectorException) as ei:
        _parser([_path("STRING:city.name")], [("GeoIPCityDissector", "Does not exist")], fmt="%h").parse_batch(b"x\n")
    assert "Does not exist (No such file or directory)" in str(ei.value) and "GeoIPCityDissector" in str(ei.value)
    p = _parser(fields_of("GeoIPCityDissector") + fields_of("GeoIPASNDissector"),
                [("GeoIPCityDissector", city), ("GeoIPASNDissector", asn)], fmt="%h")
    r = p.parse_batch(b"80.100.47.45\n2001:980:91c0:1:21c:c0ff:fe06:e580\n1.2.3.4\n127.0.0.1\nlocalhost\n-\n")
    assert p.device_program_ok, p.unsupported_reason
    assert r.status.tolist() == [lpa.LINE_OK] * 4 + [lpa.LINE_FALLBACK, lpa.LINE_OK]
    rec = r.record(0)
    assert rec[_path("STRING:city.name")] == ["Amstelveen"] and rec[_path("NUMBER:city.confidence")] == [{"l": 1}]
    assert rec[_path("STRING:location.latitude")] == ["52.5"] and rec[_path("ASN:asn.number")] == [{"l": 4444}]
    assert r.record(1)[_path("ASN:asn.number")] == [{"l": 6666}] and r.record(1)[_path("NUMBER:location.metrocode")] == [{"l": 15}]
    assert r.record(2) == {} and r.record(3) == {} and r.record(5) == {}
    lat = r.table_device([(_path("STRING:location.latitude"), float)])[_path("STRING:location.latitude")]
    assert _np(lat[0])[:2].tolist() == [52.5, 52.5] and _np(lat[1]).tolist() == [1, 1, 0, 0, 0, 0]
    assert p.get_casts(_path("STRING:location.latitude")) == lpa.CAST_STRING | lpa.CAST_DOUBLE
    assert p.get_casts(_path("ASN:asn.number")) == lpa.CAST_STRING | lpa.CAST_LONG
    got = {}
    q = lpa.HttpdLoglineParser("%h").add_dissector("nl.basjes.parse.httpdlog.dissectors.geoip.GeoIPCityDissector", city)
    q.add_parse_target(_path("STRING:location.latitude"), setter=lambda v: got.__setitem__("lat", v), value_class=float)
    q.add_parse_target(_path("STRING:location.longitude"), setter=lambda v: got.__setitem__("lon", v), value_class=str)
    q.add_parse_target(_path("NUMBER:city.geonameid"), setter=lambda v: got.__setitem__("id", v), value_class=int)
    q.parse("80.100.47.45", object())
    assert got == {"lat": 52.5, "lon": "5.75", "id": 1234}
