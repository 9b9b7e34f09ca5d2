"""The GeoIP dissectors (hp/dissectors/geoip) on the CPU: the planner, the
MaxMind DB reader, the address parser and the tree walk through the emulation
of the device's per-line code (tests/emu/geoip_emu.cpp), against
  * the expectations of the reference's TestGeoIPDissectors.java
    (tests/golden/geoip_vectors.json), and
  * an independent Python restatement (tests/geoip_ref.py) on synthetic
    databases and a 1,000-line corpus (tests/geoip_corpus.py): every line,
    every output, and FALLBACK on exactly the planted lines."""
import json
import os
import random

import pytest

import geoip_corpus as gc
import geoip_emu_lib as ge
import geoip_ref as gr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "geoip")
VECTORS = json.load(open(os.path.join(HERE, "golden", "geoip_vectors.json")))
PREFIX = "connection.client.host."
CITY_DB = os.path.join(GOLD, "GeoIP2-City-Test.mmdb")
COUNTRY_DB = os.path.join(GOLD, "GeoIP2-Country-Test.mmdb")
ASN_DB = os.path.join(GOLD, "GeoLite2-ASN-Test.mmdb")
ISP_DB = os.path.join(GOLD, "GeoIP2-ISP-Test.mmdb")


def fields_of(cls, prefix=PREFIX):
    return ["%s:%s%s" % (n.split(":")[0], prefix, n.split(":")[1]) for n, _, _ in gr.CLASSES[cls]]


def expected_record(out, prefix=PREFIX):
    """geoip_ref.dissect's outputs as the emulation's canonical record"""
    rec = {}
    for name, v in out.items():
        t, n = name.split(":")
        rec["%s:%s%s" % (t, prefix, n)] = [None if v is None else v if isinstance(v, str) else {"l": v}]
    return rec


# ---- the reference's own vectors ----------------------------------------------
@pytest.mark.parametrize("case", VECTORS["cases"], ids=lambda c: c["name"])
def test_golden_prefix_form(case):
    """the "%h" parser form (TestGeoIPDissectorsWithPrefix): outputs below connection.client.host"""
    path = os.path.join(GOLD, case["database"])
    wanted = sorted({o for o, _ in case.get("expect", [])} | set(case.get("absent", [])))
    fields = ["%s:%s%s" % (o.split(":")[0], PREFIX, o.split(":")[1]) for o in wanted] or fields_of(case["class"])
    if "error" in case:
        with pytest.raises(ge.CompileError) as ei:
            ge.Emu("%h", fields_of(case["class"]), dissectors=[(case["class"], case["database"])])
        assert ei.value.status == ge.LP_E_INVALID
        assert case["message_contains"] in ei.value.msg and case["class"] in ei.value.msg
        with pytest.raises(ge.CompileError):
            ge.possible_paths("%h", dissectors=[(case["class"], case["database"])])
        return
    e = ge.Emu("%h", fields, dissectors=[(case["class"], path)])
    assert e.status == 0, e.err
    (st, rec, _), = e.parse_batch(case["input"].encode() + b"\n")
    assert st == ge.OK
    for out, want in case.get("expect", []):
        key = "%s:%s%s" % (out.split(":")[0], PREFIX, out.split(":")[1])
        got = rec[key]
        assert len(got) == 1
        if "string" in want:  # Value.getString: a long's decimal text, a double's Double.toString
            assert (got[0] if isinstance(got[0], str) else str(got[0]["l"])) == want["string"], key
        elif "long" in want:
            assert got[0] == {"l": want["long"]} and e.casts(key) & 2, key
        else:  # a DOUBLE output: delivered as its text, cast STRING | DOUBLE
            assert float(got[0]) == want["double"] and e.casts(key) == 5, key
    for out in case.get("absent", []):
        assert "%s:%s%s" % (out.split(":")[0], PREFIX, out.split(":")[1]) not in rec


@pytest.mark.parametrize("case", [c for c in VECTORS["cases"] if "error" not in c], ids=lambda c: c["name"])
def test_golden_bare_form(case):
    """the bare dissector form (no parser around it, no prefix): the values
    the class reads for the input, which the independent restatement must
    find in the file too -- it is the reference of every corpus test below"""
    rd = gr.Reader(open(os.path.join(GOLD, case["database"]), "rb").read())
    out = gr.dissect(rd, case["class"], case["input"])
    for name, want in case.get("expect", []):
        if "string" in want:
            assert str(out[name]) == want["string"], name
        elif "long" in want:
            assert out[name] == want["long"], name
        else:
            assert float(out[name]) == want["double"], name
    for name in case.get("absent", []):
        assert name not in out


# ---- synthetic databases x the corpus ------------------------------------------
@pytest.fixture(scope="module")
def lines():
    return gc.corpus()


@pytest.fixture(scope="module")
def baseline(lines):
    """today's program, without GeoIP: the status of every line"""
    e = ge.Emu(gc.LOGFORMAT, ["IP:connection.client.host"])
    return [st for st, _, _ in e.parse_batch(gc.data_of(lines))]


def check_corpus(e, rd, cls, lines, baseline, prefix=PREFIX):
    got = e.parse_batch(gc.data_of(lines))
    assert len(got) == len(lines)
    planted, fallback = set(), set()
    for k, ((line, host), (st, rec, geo)) in enumerate(zip(lines, got)):
        if st == ge.FALLBACK and baseline[k] != ge.FALLBACK:
            fallback.add(k)
        if host is None or baseline[k] != ge.OK:
            assert st == baseline[k], (k, line[:80])
            continue
        want = gr.dissect(rd, cls, None if host == "-" else host)
        if want is None:
            planted.add(k)
            continue
        assert st == ge.OK, (k, host)
        rec.pop("IP:connection.client.host", None)
        assert rec == expected_record(want, prefix), (k, host)
        assert (geo[0] != 0) == bool(want), (k, host)
    assert fallback == planted  # FALLBACK on exactly the planted lines
    return planted


@pytest.mark.parametrize("name", sorted(gc.CITY_DBS))
def test_corpus_city(tmp_path, name, lines, baseline):
    path, data, _ = gc.write_db(tmp_path, name)
    rd = gr.Reader(data)
    e = ge.Emu(gc.LOGFORMAT, fields_of("GeoIPCityDissector") + ["IP:connection.client.host"],
               dissectors=[("GeoIPCityDissector", path)])
    assert e.status == 0, e.err
    planted = check_corpus(e, rd, "GeoIPCityDissector", lines, baseline)
    hosts = {lines[k][1] for k in planted}
    assert set(gc.UNDECIDED_HOSTS) <= hosts
    if rd.ip_version == 6:
        assert hosts == set(gc.UNDECIDED_HOSTS)
    else:  # an IPv6 address against an ip_version 4 database is the reference's line too
        assert "2001:db8::1.2.3.4" in hosts and "::ffff:1.2.3.4" not in hosts and "::" in hosts


def test_corpus_planted_lines_are_not_fallback_without_geoip(lines, baseline):
    ok = [k for k, (_, h) in enumerate(lines) if h is not None]
    assert all(baseline[k] == ge.OK for k in ok)
    assert {baseline[k] for k, (_, h) in enumerate(lines) if h is None} == {ge.BAD, ge.FALLBACK}


def test_tree_shapes(tmp_path):
    """the shapes the corpus databases were built for, one by one"""
    def ids(name, hosts):
        path, data, _ = gc.write_db(tmp_path, name)
        rd = gr.Reader(data)
        e = ge.Emu("%h", ["STRING:connection.client.host.city.name"], dissectors=[("GeoIPCityDissector", path)])
        got = e.parse_batch(b"".join(h.encode() + b"\n" for h in hosts))
        for h, (st, rec, geo) in zip(hosts, got):
            want = gr.dissect(rd, "GeoIPCityDissector", h)
            assert st == (ge.FALLBACK if want is None else ge.OK), h
            assert want is None or (geo[0] != 0) == bool(want), h
        return [g[0] for _, _, g in got]
    # the mapped text is looked up as IPv4: the record of ::1.2.3.4, not the one at ::ffff:1.2.3.4
    a = ids("v6_28", ["1.2.3.4", "::ffff:1.2.3.4", "::1.2.3.4", "::ffff:102:304", "1.2.3.5"])
    assert a[0] and a[0] == a[1] == a[2] == a[3] and a[4] == 0
    # no ::/96: every IPv4 address is none
    assert ids("v6_32_big", ["1.2.3.4", "0.0.0.0", "255.255.255.255", "::ffff:9.9.9.9"]) == [0, 0, 0, 0]
    # ::/64 is a record: the IPv4 start is a leaf already
    b = ids("v6_leaf64", ["0.0.0.0", "255.255.255.255", "::1", "::", "0:0:0:1::", "1::"])
    assert b[0] and b[0] == b[1] == b[2] == b[3] and b[4] not in (0, b[0]) and b[5] == 0
    # prefix lengths 1, 31, 32 of an ip_version 4 tree
    c = ids("v4_24", ["128.0.0.0", "255.255.255.255", "1.2.3.4", "1.2.3.5", "1.2.3.6", "1.2.3.7", "0.0.0.0", "0.0.0.1",
                      "127.255.255.255", "127.255.255.254"])
    assert c[0] == c[1] != 0 and c[2] == c[3] != 0 and c[4] not in (0, c[2]) and c[5] == 0 and c[6] and not c[7]
    assert c[8] and not c[9]


def test_corpus_asn_and_two_databases(tmp_path, lines, baseline):
    """two classes, two databases, one handle: City and ASN on the same token"""
    cpath, cdata, _ = gc.write_db(tmp_path, "v6_28")
    apath, adata, _ = gc.write_db(tmp_path, "asn")
    crd, ard = gr.Reader(cdata), gr.Reader(adata)
    sub = lines[:300]
    e = ge.Emu(gc.LOGFORMAT, fields_of("GeoIPCityDissector") + fields_of("GeoIPASNDissector"),
               dissectors=[("GeoIPCityDissector", cpath), ("nl.basjes.parse.httpdlog.dissectors.geoip.GeoIPASNDissector", apath)])
    assert e.status == 0, e.err
    got = e.parse_batch(gc.data_of(sub))
    for k, ((line, host), (st, rec, geo)) in enumerate(zip(sub, got)):
        if host is None:
            assert st == baseline[k]
            continue
        h = None if host == "-" else host
        wc, wa = gr.dissect(crd, "GeoIPCityDissector", h), gr.dissect(ard, "GeoIPASNDissector", h)
        if wc is None:
            assert st == ge.FALLBACK and wa is None
            continue
        assert st == ge.OK and rec == expected_record(dict(wc, **wa)), (k, host)


def test_wave_edge_cuts(tmp_path, lines, baseline):
    path, data, _ = gc.write_db(tmp_path, "v6_28")
    rd = gr.Reader(data)
    e = ge.Emu(gc.LOGFORMAT, fields_of("GeoIPCityDissector"), dissectors=[("GeoIPCityDissector", path)])
    for n in (1, 63, 64, 65, 129):
        check_corpus(e, rd, "GeoIPCityDissector", lines[:n], baseline[:n])


def test_remapped_header_token(tmp_path):
    """a header token remapped to IP is a source too"""
    path, data, _ = gc.write_db(tmp_path, "v6_28")
    rd = gr.Reader(data)
    p = "request.header.x-forwarded-for."
    e = ge.Emu('%h "%{X-Forwarded-For}i"', ["STRING:" + p + "city.name", "NUMBER:" + p + "city.geonameid"],
               remaps=[("request.header.x-forwarded-for", "IP")], dissectors=[("GeoIPCityDissector", path)])
    assert e.status == 0, e.err
    got = e.parse_batch(b'9.9.9.9 "80.100.1.2"\n9.9.9.9 "-"\nlocalhost "1::5"\n9.9.9.9 "proxy.example"\n')
    assert [st for st, _, _ in got] == [ge.OK, ge.OK, ge.OK, ge.FALLBACK]
    w = gr.dissect(rd, "GeoIPCityDissector", "80.100.1.2")
    assert got[0][1] == {"STRING:" + p + "city.name": [w["STRING:city.name"]],
                         "NUMBER:" + p + "city.geonameid": [{"l": w["NUMBER:city.geonameid"]}]}
    assert got[1][1] == {}
    assert got[2][1]["STRING:" + p + "city.name"] == ["Shared City Name"]


def test_two_formats_one_with_the_stage(tmp_path):
    path, data, _ = gc.write_db(tmp_path, "v6_28")
    e = ge.Emu('%h %l %u\n%u "%{Referer}i"', ["STRING:connection.client.host.city.name", "STRING:connection.client.user"],
               dissectors=[("GeoIPCityDissector", path)])
    assert e.status == 0, e.err
    got = e.parse_batch(b'80.100.1.2 - alice\nbob "http://x/"\nlocalhost - carol\ndave "-"\n')
    assert [st for st, _, _ in got] == [ge.OK, ge.OK, ge.FALLBACK, ge.OK]
    assert got[0][1]["STRING:connection.client.host.city.name"] and got[0][2][0] != 0
    assert "STRING:connection.client.host.city.name" not in got[1][1] and got[1][2][0] == 0


# ---- the planner ---------------------------------------------------------------
def test_possible_paths():
    without = ge.possible_paths("%h")
    assert not [p for p in without if ".country." in p or ".asn." in p]
    with_city = ge.possible_paths("%h %a", dissectors=[("GeoIPCityDissector", CITY_DB)])
    for base in ("connection.client.host", "connection.client.ip"):  # below every IP-typed path
        for n, _, _ in gr.CITY:
            assert "%s:%s.%s" % (n.split(":")[0], base, n.split(":")[1]) in with_city
    assert not [p for p in with_city if ".asn." in p]
    isp = ge.possible_paths("$remote_addr", dissectors=[("GeoIPISPDissector", ISP_DB)])
    assert {"ASN:connection.client.host.asn.number", "STRING:connection.client.host.isp.name"} <= set(isp)
    remapped = ge.possible_paths('"%{X-Real-IP}i"', remaps=[("request.header.x-real-ip", "IP")],
                                 dissectors=[("GeoIPCountryDissector", COUNTRY_DB)])
    assert "STRING:request.header.x-real-ip.country.name" in remapped


def test_casts():
    e = ge.Emu("%h", fields_of("GeoIPCityDissector"), dissectors=[("GeoIPCityDissector", CITY_DB)])
    for n, kind, _ in gr.CITY:
        assert e.casts("%s:%s%s" % (n.split(":")[0], PREFIX, n.split(":")[1])) == gr.CASTS[kind], n
    e = ge.Emu("%h", fields_of("GeoIPISPDissector"), dissectors=[("GeoIPISPDissector", ISP_DB)])
    for n, kind, _ in gr.ISP:
        assert e.casts("%s:%s%s" % (n.split(":")[0], PREFIX, n.split(":")[1])) == gr.CASTS[kind], n


def compile_status(fmt, fields, dissectors, remaps=()):
    try:
        e = ge.Emu(fmt, fields, remaps=remaps, dissectors=dissectors)
        return e.status, e.err
    except ge.CompileError as x:
        return x.status, x.msg


def test_registration_errors():
    f = ["STRING:connection.client.host.country.name"]
    assert compile_status("%h", f, [("GeoIPCityDissector", "")])[0] == ge.LP_E_INVALID
    st, msg = compile_status("%h", f, [("GeoIPCityDissector", "/no/such/file.mmdb")])
    assert st == ge.LP_E_INVALID and "GeoIPCityDissector" in msg and "/no/such/file.mmdb" in msg
    st, msg = compile_status("%h", f, [("GeoIPCityDissector", __file__)])  # a file, but no database
    assert st == ge.LP_E_INVALID and __file__ in msg
    assert compile_status("%h", f, [("GeoIPTownDissector", CITY_DB)])[0] == ge.LP_E_INVALID
    assert compile_status("%h", f, [("nl.basjes.parse.httpdlog.dissectors.GeoIPCityDissector", CITY_DB)])[0] == ge.LP_E_INVALID
    # twice with the same path is once; with different paths unsupported
    assert compile_status("%h", f, [("GeoIPCityDissector", CITY_DB)] * 2)[0] == 0
    assert compile_status("%h", f, [("GeoIPCityDissector", CITY_DB), ("GeoIPCityDissector", COUNTRY_DB)])[0] == ge.LP_E_UNSUPPORTED
    # a database of another type
    st, msg = compile_status("%h", f, [("GeoIPCityDissector", COUNTRY_DB)])
    assert st == ge.LP_E_UNSUPPORTED and "Country" in msg
    # a path two registered classes deliver from the same input
    st, msg = compile_status("%h", f, [("GeoIPCityDissector", CITY_DB), ("GeoIPCountryDissector", COUNTRY_DB)])
    assert st == ge.LP_E_UNSUPPORTED and "connection.client.host.country.name" in msg
    st, msg = compile_status("%h", ["ASN:connection.client.host.asn.number"],
                             [("GeoIPISPDissector", ISP_DB), ("GeoIPASNDissector", ASN_DB)])
    assert st == ge.LP_E_UNSUPPORTED and "connection.client.host.asn.number" in msg
    # ... but not when they deliver different paths
    assert compile_status("%h", f + ["ASN:connection.client.host.asn.number"],
                          [("GeoIPCountryDissector", COUNTRY_DB), ("GeoIPASNDissector", ASN_DB)])[0] == 0
    # without registration the path does not exist
    assert compile_status("%h", f, [])[0] == ge.LP_E_MISSING


def test_unsupported_sources():
    d = [("GeoIPCountryDissector", COUNTRY_DB)]
    # a query parameter remapped to IP
    st, msg = compile_status('%h "%r"', ["STRING:request.firstline.uri.query.ip.country.name"], d,
                             remaps=[("request.firstline.uri.query.ip", "IP")])
    assert st == ge.LP_E_UNSUPPORTED and msg
    # $binary_remote_addr's derived value
    st, msg = compile_status("$binary_remote_addr", ["STRING:connection.client.host.country.name"], d)
    assert st == ge.LP_E_UNSUPPORTED and msg
    # the address of a mod_unique_id
    st, msg = compile_status('%h "%{unique_id}e"', ["STRING:server.environment.unique_id.ip.country.name"], d,
                             remaps=[("server.environment.unique_id", "MOD_UNIQUE_ID")])
    assert st == ge.LP_E_UNSUPPORTED and msg


def test_value_budget(tmp_path):
    """GeoIP stages share the eight value stages"""
    hdrs = ["x-ip-%d" % k for k in range(9)]
    fmt = " ".join('"%%{%s}i"' % h for h in hdrs)
    remaps = [("request.header." + h, "IP") for h in hdrs]
    d = [("GeoIPCountryDissector", COUNTRY_DB)]
    f = ["STRING:request.header.%s.country.iso" % h for h in hdrs]
    assert compile_status(fmt, f[:8], d, remaps)[0] == 0
    st, msg = compile_status(fmt, f, d, remaps)
    assert st == ge.LP_E_UNSUPPORTED and "at most 8" in msg


# ---- damaged databases ------------------------------------------------------------
def test_damaged_database_is_invalid_never_a_crash(tmp_path):
    good = open(CITY_DB, "rb").read()
    f = fields_of("GeoIPCityDissector")
    rnd = random.Random(7)
    cuts = [0, 1, 13, 14, 15, 100, len(good) // 2, len(good) - 200, len(good) - 30, len(good) - 1]
    seen = set()
    for k, n in enumerate(cuts):
        p = tmp_path / ("cut%d.mmdb" % k)
        p.write_bytes(good[:n])
        st, msg = compile_status("%h", f, [("GeoIPCityDissector", str(p))])
        assert st == ge.LP_E_INVALID, (n, st, msg)  # (the metadata ends the file: every cut loses it)
    for k in range(120):
        b = bytearray(good)
        # the tree, the data section and the metadata in turn
        lo, hi = ((0, 2835), (2835, len(good) - 150), (len(good) - 150, len(good)))[k % 3]
        for _ in range(1 + k % 4):
            b[rnd.randrange(lo, hi)] ^= 1 << rnd.randrange(8)
        p = tmp_path / "flip.mmdb"
        p.write_bytes(bytes(b))
        try:
            e = ge.Emu("%h", f, dissectors=[("GeoIPCityDissector", str(p))])
        except ge.CompileError as x:
            assert x.status == ge.LP_E_INVALID
            seen.add(x.status)
            continue
        seen.add(e.status)
        assert e.status in (0, ge.LP_E_UNSUPPORTED)
        if e.status == 0:  # still a database: lookups must stay inside it
            for st, _, _ in e.parse_batch(b"80.100.47.45\n2001:980:91c0:1:21c:c0ff:fe06:e580\n1.2.3.4\n::\n"):
                assert st == ge.OK
    assert ge.LP_E_INVALID in seen and 0 in seen
