"""ScreenResolutionDissector and ModUniqueIdDissector on type-remapped values,
GPU part: the guard in k_derived_lines (a repeated parameter, a missing part of
split("x")) and the values in the table kernels (table_value.h TC_SCREEN /
TC_UNIQUEID), on the corpus of remap_dissector_corpus.py.  Two handles: A is
today's program (the same format, remaps and fields without the new outputs),
B adds the new outputs.  A must be the oracle's and never FALLBACK on this
corpus; B's statuses differ from A's exactly where the Python restatement
(remap_dissector_ref.py) raises or a parameter repeats, and every new column
equals the expectation exactly -- values, validity, offsets and bytes, from the
device view, the host copy and the emit stream.  The CPU part is
test_remap_dissectors.py."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import logparser_amd as lpa
import oracle_lib
import remap_dissector_corpus as rc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOURCES = (rc.P_S, rc.P_UID, rc.T_UID, rc.T_RES)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _parser(fields, remaps=rc.REMAPS, dissectors=rc.DISSECTORS, fmt=rc.LOGFORMAT):
    p = lpa.HttpdLoglineParser(fmt, list(fields))
    for name, settings in dissectors:
        p.add_dissector(name, settings)
    for path, typ in remaps:
        p.add_type_remapping(path, typ)
    return p


@functools.lru_cache(None)
def _corpus():
    """the corpus parsed by both handles (each keeps its batch: one batch per handle), and the expectations"""
    data, lines = rc.corpus()
    pa, pb = _parser(rc.FIELDS_A), _parser(rc.FIELDS_B)
    ra, rb = pa.parse_batch(data), pb.parse_batch(data)
    assert pa.device_program_ok and pb.device_program_ok, (pa.unsupported_reason, pb.unsupported_reason)
    assert ra.n_lines == rb.n_lines == len(lines) == 1000
    exp = [rc.expected(ln) for ln in lines]
    return data, lines, exp, ra, rb


def _expected_column(exp, field, typ):
    """(valid, values) of a new column: STRING values as text, LONG as ints"""
    conv = rc.as_string if typ is str else rc.as_long
    vals = [None if e is None or field not in e else conv(e[field]) for e in exp]
    return np.array([v is not None for v in vals], dtype=bool), vals


def _same_string(got, valid, vals, what):
    """an Arrow STRING column (offsets, chars), valid against the expectation: exact offsets and bytes"""
    (off, chars), ok = got
    off, chars, ok = _np(off).astype(np.int64), _np(chars), _np(ok).astype(bool)
    assert ok.tolist() == valid.tolist(), (what, "valid")
    enc = [v.encode() if v is not None else b"" for v in vals]
    want_off = np.concatenate([[0], np.cumsum([len(b) for b in enc])]).astype(np.int64)
    assert off.tolist() == want_off.tolist(), (what, "offsets")
    assert chars.tobytes()[:want_off[-1]] == b"".join(enc), (what, "bytes")


def _same_long(got, valid, vals, what):
    x, ok = got
    x, ok = _np(x), _np(ok).astype(bool)
    assert ok.tolist() == valid.tolist(), (what, "valid")
    assert [int(x[k]) for k in range(len(vals)) if valid[k]] == [v for v in vals if v is not None], (what, "values")


def test_handle_a_is_the_oracles_and_never_fallback_gpu():
    data, lines, exp, ra, rb = _corpus()
    assert ra.status.tolist() == [lpa.LINE_OK] * 1000
    assert ra.counters["fallback"] == 0 and ra.counters["ok"] == 1000
    o = oracle_lib.Oracle(rc.LOGFORMAT, rc.FIELDS_A, rc.REMAPS)
    for i, line in enumerate(data.decode().split("\n")[:-1]):
        st, js = o.parse_raw(line)
        assert st == oracle_lib.OK and js == ra.record_json(i), i


def test_status_rule_gpu():
    """status_B is FALLBACK exactly where status_A is OK and the Python rule raises or a parameter repeats"""
    _, lines, exp, ra, rb = _corpus()
    want = [lpa.LINE_FALLBACK if e is None and ra.status[i] == lpa.LINE_OK else int(ra.status[i]) for i, e in enumerate(exp)]
    assert rb.status.tolist() == want
    n_fb = want.count(lpa.LINE_FALLBACK)
    assert n_fb == rc.planted_fallbacks(lines) == rb.counters["fallback"]
    assert rb.counters["ok"] == 1000 - n_fb and rb.counters["bad"] == 0


def test_shared_fields_identical_gpu():
    _, lines, exp, ra, rb = _corpus()
    cols = [(f, str) for f in rc.FIELDS_A]
    ta, tb = ra.table_device(cols), rb.table_device(cols)
    _, res_b = rb.copy_to_host()
    hb = rb.table_from(res_b, cols, decode=False)
    okb = np.array([e is not None for e in exp])
    for f in rc.FIELDS_A:
        (oa, ca), va = ta[f]
        oa, ca, va = _np(oa), _np(ca).tobytes(), _np(va).astype(bool)
        vals = [ca[oa[k]:oa[k + 1]].decode() if va[k] and okb[k] else None for k in range(1000)]
        valid = va & okb
        _same_string(tb[f], valid, vals, (f, "device"))
        _same_string(hb[f], valid, vals, (f, "host"))


def test_new_columns_device_and_host_gpu():
    """every new output as a STRING and as a LONG column, from lp_result_table on the device view and on the host copy"""
    _, lines, exp, ra, rb = _corpus()
    assert len(rc.NEW_FIELDS) == 14
    dev_s = rb.table_device([(f, str) for f in rc.NEW_FIELDS])
    dev_l = rb.table_device([(f, int) for f in rc.NEW_FIELDS])
    _, res = rb.copy_to_host()
    host_s = rb.table_from(res, [(f, str) for f in rc.NEW_FIELDS], decode=False)
    host_l = rb.table_from(res, [(f, int) for f in rc.NEW_FIELDS])
    for f in rc.NEW_FIELDS:
        valid, vals = _expected_column(exp, f, str)
        assert valid.sum() > 20, f
        _same_string(dev_s[f], valid, vals, (f, "device"))
        _same_string(host_s[f], valid, vals, (f, "host"))
        valid, vals = _expected_column(exp, f, int)
        _same_long(dev_l[f], valid, vals, (f, "device"))
        _same_long(host_l[f], valid, vals, (f, "host"))
    # an address has no long; a part that is no number neither (" 800", "", 2^63)
    assert not _expected_column(exp, "IP:%s.ip" % rc.T_UID, int)[0].any()
    vs, _ = _expected_column(exp, "SCREENHEIGHT:%s.height" % rc.P_S, str)
    vl, _ = _expected_column(exp, "SCREENHEIGHT:%s.height" % rc.P_S, int)
    assert (vs & ~vl).sum() > 20


def test_emit_stream_gpu():
    """lp_result_emit: the new outputs in the reference's delivery order (width, height; epoch, ip, processid,
    counter, threadindex), per source in the order the sources are delivered"""
    _, lines, exp, ra, rb = _corpus()
    _, res = rb.copy_to_host()
    types = {f.split(":")[0] for f in rc.NEW_FIELDS}
    for i, e in enumerate(exp):
        if e is None:
            continue
        got = [(b, t, n, v) for b, t, n, v in rb.emissions_from(res, i) if t in types and b in SOURCES]
        want = [(f.split(":")[1].rsplit(".", 1)[0], f.split(":")[0], f.rsplit(".", 1)[1], e[f]) for f in rc.NEW_FIELDS if f in e]
        assert got == want, i
        rec = rb.record(i)
        for f in rc.NEW_FIELDS:
            v = [x for x in rec.get(f, []) if x is not None]
            assert ([x["l"] if isinstance(x, dict) else x for x in v] or [None])[-1] == e.get(f), (i, f)


def test_rows_dict_and_arrow_gpu():
    """lp_result_table_rows over the OK rows, a dictionary column and an Arrow batch of all seven new types"""
    import pyarrow as pa
    _, lines, exp, ra, rb = _corpus()
    ok = [i for i, e in enumerate(exp) if e is not None]
    rows = rb.select_device(lpa.SEL_OK)
    assert _np(rows).tolist() == ok
    exp_ok = [exp[i] for i in ok]
    fs = ["SCREENWIDTH:%s.width" % rc.T_RES, "TIME.EPOCH:%s.epoch" % rc.P_UID, "IP:%s.ip" % rc.P_UID]
    t = rb.table_device([(f, str) for f in fs], rows=rows)
    for f in fs:
        valid, vals = _expected_column(exp_ok, f, str)
        _same_string(t[f], valid, vals, (f, "rows"))
    # one dictionary column: the addresses of the token's ids
    ipf = "IP:%s.ip" % rc.T_UID
    valid, vals = _expected_column(exp, ipf, str)
    for kw, want_valid, want_vals in (({}, valid, vals), ({"rows": rows}, valid[ok], [vals[i] for i in ok])):
        index, (doff, dchars), dvalid = rb.table_dict_device([ipf], **kw)[ipf]
        got = lpa.strings_from_dict(_np(dvalid), _np(index), _np(doff), _np(dchars))
        assert [g if want_valid[k] else None for k, g in enumerate(got)] == want_vals
        assert _np(dvalid).astype(bool).tolist() == want_valid.tolist()
        ents = len(_np(doff)) - 1
        assert ents == len({v for v in want_vals if v is not None})
    # one Arrow batch holding all seven new types
    cols = [("SCREENWIDTH:%s.width" % rc.P_S, int, "w"), ("SCREENHEIGHT:%s.height" % rc.P_S, str, "h"),
            ("TIME.EPOCH:%s.epoch" % rc.T_UID, int, "epoch"), (ipf, "dict", "ip"),
            ("PROCESSID:%s.processid" % rc.T_UID, int, "pid"), ("COUNTER:%s.counter" % rc.T_UID, str, "counter"),
            ("THREAD_INDEX:%s.threadindex" % rc.T_UID, int, "thread")]
    ex = rb.to_arrow_device(cols)
    try:
        batch = ex.to_host()
    finally:
        ex.release()
    assert isinstance(batch, pa.RecordBatch) and batch.num_rows == 1000
    batch.validate(full=True)
    for path, typ, name in cols:
        _, vals = _expected_column(exp, path, int if typ is int else str)
        assert batch.column(batch.schema.get_field_index(name)).to_pylist() == vals, name


def test_width_only_gpu():
    """the throw depends on what is requested: "1280x" lines are OK with only the width, FALLBACK with the height added"""
    data, lines, exp, ra, rb = _corpus()
    wf = ["SCREENWIDTH:%s.width" % rc.P_S, "SCREENWIDTH:%s.width" % rc.T_RES]
    p = _parser(rc.FIELDS_A + wf)
    r = p.parse_batch(data)
    expw = [rc.expected(ln, True, False, want_uid=False) for ln in lines]
    assert r.status.tolist() == [lpa.LINE_FALLBACK if e is None else lpa.LINE_OK for e in expw]
    flipped = [i for i in range(1000) if expw[i] is not None and exp[i] is None and not lines[i]["uid_twice"]]
    assert len(flipped) > 20 and all(rb.status[i] == lpa.LINE_FALLBACK for i in flipped)
    t = r.table_device([(f, str) for f in wf])
    for f in wf:
        valid, vals = _expected_column(expw, f, str)
        _same_string(t[f], valid, vals, f)


def _golden_cases():
    doc = json.load(open(os.path.join(GOLDEN, "remap_dissector_vectors.json")))
    for c in doc["cases"]:
        if "line_file" in c:
            c["line"] = open(os.path.join(GOLDEN, c["line_file"])).read().rstrip("\n")
    return doc["cases"]


@pytest.mark.parametrize("case", _golden_cases(), ids=lambda c: c["name"])
def test_golden_vectors_gpu(case):
    p = _parser(case["fields"], [tuple(r) for r in case["remaps"]], [tuple(d) for d in case["dissectors"]], case["logformat"])
    r = p.parse_batch((case["line"] + "\n").encode())
    assert p.device_program_ok, p.unsupported_reason
    assert r.status.tolist() == [lpa.LINE_OK]
    rec = r.record(0)
    dev = r.table_device([(f, str) for f in case["fields"]])
    longs = r.table_device([(f, int) for f in case["long"]]) if case["long"] else {}
    for f in case["fields"]:
        (off, chars), valid = dev[f]
        got = _np(chars).tobytes()[: int(_np(off)[1])].decode() if _np(valid)[0] else None
        assert got == case["expect"].get(f), f
        assert (f in case["absent"]) <= (got is None and not [x for x in rec.get(f, []) if x is not None])
        if f in case["long"]:
            x, ok = longs[f]
            assert _np(ok)[0] and int(_np(x)[0]) == int(case["expect"][f]), f
            assert p.get_casts(f) & lpa.CAST_LONG


def test_nested_source_gpu():
    """a parameter of a derived URI's query (…query.g.query.s), 64 lines: one full wave.  The guard runs on the
    device after the derived URI stages.  Two sources deliver the path -- the nested parameter, and a parameter of
    the request itself that is literally named "g.query.s" -- so its columns are the host table's (a path two
    sources deliver is left to the replay, which knows the line's delivery order)."""
    data, exp = rc.nested_corpus()
    p = _parser(rc.NESTED_FIELDS, rc.NESTED_REMAPS)
    r = p.parse_batch(data)
    assert p.device_program_ok, p.unsupported_reason
    assert r.status.tolist() == [lpa.LINE_FALLBACK if e is None else lpa.LINE_OK for e in exp]
    assert r.counters["fallback"] == sum(e is None for e in exp) > 10
    _, res = r.copy_to_host()
    t = r.table_from(res, [(f, str) for f in rc.NESTED_FIELDS[1:]], decode=False)
    for f in rc.NESTED_FIELDS[1:]:
        valid, vals = _expected_column(exp, f, str)
        assert valid.any()
        _same_string(t[f], valid, vals, f)
    with pytest.raises(lpa.FallbackRequired):
        r.table_device([(rc.NESTED_FIELDS[1], str)])


def test_screen_token_without_uri_stages_gpu():
    """a program without URI, list or cookie stages (no URI kernel, no arena regions): k_derived_lines alone
    runs the token's guard and moves the batch's counters; the values from the device table"""
    data, lines, _, _, _ = _corpus()
    for want_h in (True, False):
        fields = rc.TOKEN_ONLY_FIELDS if want_h else rc.TOKEN_ONLY_FIELDS[:2]
        p = _parser(fields, rc.TOKEN_ONLY_REMAPS)
        r = p.parse_batch(data)
        assert p.device_program_ok, p.unsupported_reason
        exp = [rc.expected_token_only(ln, True, want_h) for ln in lines]
        assert r.status.tolist() == [lpa.LINE_FALLBACK if e is None else lpa.LINE_OK for e in exp]
        n_fb = sum(e is None for e in exp)
        assert n_fb > 100
        assert r.counters == {"lines": 1000, "ok": 1000 - n_fb, "bad": 0, "fallback": n_fb}
        t = r.table_device([(f, str) for f in fields[1:]])
        tl = r.table_device([(f, int) for f in fields[1:]])
        _, res = r.copy_to_host()
        th = r.table_from(res, [(f, str) for f in fields[1:]], decode=False)
        for f in fields[1:]:
            valid, vals = _expected_column(exp, f, str)
            _same_string(t[f], valid, vals, (f, "device"))
            _same_string(th[f], valid, vals, (f, "host"))
            valid, vals = _expected_column(exp, f, int)
            _same_long(tl[f], valid, vals, (f, "device"))
    # a single-token format, the batch smaller than a wave
    p = _parser(["SCREENWIDTH:request.header.x-res.width"], rc.TOKEN_ONLY_REMAPS, fmt='%h "%{X-Res}i"')
    r = p.parse_batch(b'1.2.3.4 "640x480"\n1.2.3.4 "x"\n1.2.3.4 "-"\nbad\n')
    assert p.device_program_ok, p.unsupported_reason
    assert r.status.tolist() == [lpa.LINE_OK, lpa.LINE_FALLBACK, lpa.LINE_OK, lpa.LINE_BAD]
    assert r.counters == {"lines": 4, "ok": 2, "bad": 1, "fallback": 1}
    assert r.record(0) == {"SCREENWIDTH:request.header.x-res.width": ["640"]}


def test_python_mirror_gpu():
    """add_dissector / get_possible_paths(dissectors=) / a Long setter for a new target"""
    rm = [(rc.P_S, "SCREENRESOLUTION", lpa.CAST_STRING)]
    with_d = set(lpa.get_possible_paths(rc.LOGFORMAT, remaps=rm, dissectors=["ScreenResolutionDissector"]))
    without = set(lpa.get_possible_paths(rc.LOGFORMAT, remaps=rm))
    assert with_d - without == {"SCREENWIDTH:%s.width" % rc.P_S, "SCREENHEIGHT:%s.height" % rc.P_S}
    with pytest.raises(lpa.InvalidDissectorException):
        lpa.get_possible_paths(rc.LOGFORMAT, dissectors=["NoSuchDissector"])
    p = lpa.HttpdLoglineParser(rc.LOGFORMAT).add_type_remapping(rc.P_S, "SCREENRESOLUTION")
    p.add_parse_target("SCREENWIDTH:%s.width" % rc.P_S)
    with pytest.raises(lpa.MissingDissectorsException):
        p.parse_batch(b"x\n")
    with pytest.raises(lpa.InvalidDissectorException):
        lpa.HttpdLoglineParser(rc.LOGFORMAT, ["STRING:" + rc.P_S]).add_dissector("NoSuchDissector").parse_batch(b"x\n")
    got = {}
    q = lpa.HttpdLoglineParser(rc.LOGFORMAT).add_dissector("nl.basjes.parse.httpdlog.dissectors.ScreenResolutionDissector")
    q.add_type_remapping(rc.P_S, "SCREENRESOLUTION")
    q.add_parse_target("SCREENWIDTH:%s.width" % rc.P_S, setter=lambda v: got.__setitem__("w", v), value_class=int)
    q.add_parse_target("SCREENHEIGHT:%s.height" % rc.P_S, setter=lambda v: got.__setitem__("h", v), value_class=str)
    q.parse('1.2.3.4 - - [05/Sep/2010:11:27:50 +0200] "GET /?s=1280x800 HTTP/1.1" 200 5 "-" "a" "-" "-"', object())
    assert got == {"w": 1280, "h": "800"}
    assert ctypes.sizeof(lpa.LpDissector) == 2 * ctypes.sizeof(ctypes.c_void_p)
