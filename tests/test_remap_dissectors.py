"""ScreenResolutionDissector and ModUniqueIdDissector on type-remapped values
(hp/dissectors/ScreenResolutionDissector.java:32-93, ModUniqueIdDissector.java:
43-239) -- CPU tests: the planner (plan.cpp) and the per-line device code
(lp_device.h derived_line's guard, the replay's values) through the test-only
emulation with added dissectors (dissectors_emu_lib.py), against

  * the reference's own expectations (tests/golden/remap_dissector_vectors.json),
  * an independent Python restatement (remap_dissector_ref.py) on the corpus
    the GPU tests use (remap_dissector_corpus.py), every line,

and the pure split / base64 functions (csrc/lp_value.h) in a stand-alone
program under ASan + UBSan.  The GPU part is test_remap_dissectors_gpu.py.
"""
import json
import os
import subprocess

import pytest

import dissectors_emu_lib as de
import oracle_lib
import remap_dissector_corpus as rc
import remap_dissector_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
OK, BAD, FALLBACK = 0, 1, 2
CAST_S, CAST_L = 1, 2
LP_E_INVALID, LP_E_MISSING, LP_E_UNSUPPORTED = -1, -2, -3
SCREEN = [("ScreenResolutionDissector", "")]
Q = "request.firstline.uri.query."


def golden_cases():
    doc = json.load(open(os.path.join(GOLDEN, "remap_dissector_vectors.json")))
    for c in doc["cases"]:
        if "line_file" in c:
            c["line"] = open(os.path.join(GOLDEN, c["line_file"])).read().rstrip("\n")
    return doc["cases"]


def rec_value(rec, target):
    """the last non-null value the record holds for target (ParsedRecord: the last value wins), as delivered"""
    vals = [v for v in rec.get(target, []) if v is not None]
    if not vals:
        return None
    return vals[-1]["l"] if isinstance(vals[-1], dict) else vals[-1]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_golden_vectors(case):
    e = de.Emu(case["logformat"], case["fields"], [tuple(r) for r in case["remaps"]],
               [tuple(d) for d in case["dissectors"]])
    assert e.status == 0, e.err
    st, rec = e.parse(case["line"])
    assert st == OK
    for target, want in case["expect"].items():
        got = rec_value(rec, target)
        assert rc.as_string(got) == want, (target, got)
        if target in case["long"]:
            assert rc.as_long(got) == int(want), (target, got)
            assert e.casts(target) & CAST_L
    for target in case["absent"]:
        assert rec_value(rec, target) is None, target


def test_possible_paths_with_and_without_registration():
    rm = [(Q + "s", "SCREENRESOLUTION"), ("server.environment.unique_id", "MOD_UNIQUE_ID")]
    fmt = rc.LOGFORMAT
    with_d = set(de.possible_paths(fmt, 15, rm, SCREEN))
    without = set(de.possible_paths(fmt, 15, rm))
    new = {"SCREENWIDTH:" + Q + "s.width", "SCREENHEIGHT:" + Q + "s.height"}
    assert with_d - without == new
    assert "SCREENRESOLUTION:" + Q + "s" in without
    # ModUniqueIdDissector is registered by default
    for t, n in rc.UID_OUT:
        assert "%s:server.environment.unique_id.%s" % (t, n) in without
    # the fully qualified class name, and registering twice, are the same
    assert set(de.possible_paths(fmt, 15, rm, [("nl.basjes.parse.httpdlog.dissectors.ScreenResolutionDissector", "x")] * 2)) == with_d
    with pytest.raises(de.CompileError) as ei:
        de.possible_paths(fmt, 15, rm, [("GeoIPCityDissector", "")])
    assert ei.value.status == LP_E_INVALID


def test_casts_of_the_seven_targets():
    e = de.Emu(rc.LOGFORMAT, rc.FIELDS_B, rc.REMAPS, rc.DISSECTORS)
    assert e.status == 0, e.err
    for f in rc.NEW_FIELDS:
        assert e.casts(f) == CAST_S | CAST_L, f  # STRING_OR_LONG (ScreenResolutionDissector.java:81-92, ModUniqueIdDissector.java:76-100)
    assert len({f.split(":")[0] for f in rc.NEW_FIELDS}) == 7


def test_missing_without_registration():
    with pytest.raises(de.CompileError) as ei:
        de.Emu(rc.LOGFORMAT, ["SCREENWIDTH:" + Q + "s.width"], [(Q + "s", "SCREENRESOLUTION")])
    assert ei.value.status == LP_E_MISSING and "MissingDissectorsException" in ei.value.msg
    e = de.Emu(rc.LOGFORMAT, ["SCREENWIDTH:" + Q + "s.width"], [(Q + "s", "SCREENRESOLUTION")], SCREEN)
    assert e.status == 0, e.err


def test_unknown_class_is_invalid():
    with pytest.raises(de.CompileError) as ei:
        de.Emu(rc.LOGFORMAT, ["STRING:" + Q + "s"], [], [("com.example.MyDissector", "")])
    assert ei.value.status == LP_E_INVALID and "com.example.MyDissector" in ei.value.msg


def test_ninth_stage_is_unsupported():
    names = ["p%d" % k for k in range(9)]
    rm = [(Q + n, "SCREENRESOLUTION") for n in names]
    fields = ["SCREENWIDTH:%s%s.width" % (Q, n) for n in names]
    assert de.Emu(rc.LOGFORMAT, fields[:8], rm[:8], SCREEN).status == 0
    e = de.Emu(rc.LOGFORMAT, fields, rm, SCREEN)
    assert e.status == LP_E_UNSUPPORTED and "at most 8" in e.err, e.err
    assert e.parse('1.2.3.4 - - [05/Sep/2010:11:27:50 +0200] "GET /?p0=1x2 HTTP/1.1" 200 5 "-" "a" "-" "-"')[0] == FALLBACK


def test_cookie_value_source_is_unsupported():
    fmt = '%h %l %u %t "%r" %>s %b "%{Cookie}i"'
    path = "request.cookies.res"
    e = de.Emu(fmt, ["SCREENWIDTH:%s.width" % path], [(path, "SCREENRESOLUTION")], SCREEN)
    assert e.status == LP_E_UNSUPPORTED and path in e.err, e.err


def test_screen_token_without_uri_stages():
    """a SCREENRESOLUTION token in a program without URI, list or cookie stages: its guard is the only thing
    that runs after the parse kernels (k_derived_lines alone); statuses and values on the corpus' X-Res token"""
    data, lines = rc.corpus()
    for want_h in (True, False):
        fields = rc.TOKEN_ONLY_FIELDS if want_h else rc.TOKEN_ONLY_FIELDS[:2]
        e = de.Emu(rc.LOGFORMAT, fields, rc.TOKEN_ONLY_REMAPS, rc.DISSECTORS)
        assert e.status == 0, e.err
        res = e.parse_batch(data)
        n_fb = 0
        for i, ln in enumerate(lines):
            exp = rc.expected_token_only(ln, True, want_h)
            assert res[i][0] == (FALLBACK if exp is None else OK), (i, ln)
            n_fb += exp is None
            if exp is not None:
                assert rec_value(res[i][1], fields[0]) == "10.%d.%d.%d" % (i % 250, (i // 3) % 250, i % 199)
                for f in fields[1:]:
                    assert rec_value(res[i][1], f) == exp.get(f), (i, f)
        assert n_fb == sum(1 for i in range(1000) if lines[i]["tres"] in (("1280x", "x", "xx") if want_h else ("x", "xx")))
        assert n_fb > 100
    # a single-token format
    e = de.Emu('%h "%{X-Res}i"', ["SCREENWIDTH:request.header.x-res.width"], rc.TOKEN_ONLY_REMAPS, SCREEN)
    assert e.status == 0, e.err
    assert e.parse('1.2.3.4 "640x480"') == (OK, {"SCREENWIDTH:request.header.x-res.width": ["640"]})
    assert e.parse('1.2.3.4 "x"')[0] == FALLBACK and e.parse('1.2.3.4 "-"')[0] == OK


def test_settings_are_kept_but_the_separator_is_x():
    """the dissecting instance is getNewInstance()'s: it never sees the settings (core/Parser.java:424-428)"""
    fields = ["SCREENWIDTH:" + Q + "s.width", "SCREENHEIGHT:" + Q + "s.height"]
    e = de.Emu(rc.LOGFORMAT, fields, [(Q + "s", "SCREENRESOLUTION")], [("ScreenResolutionDissector", "*")])
    line = '1.2.3.4 - - [05/Sep/2010:11:27:50 +0200] "GET /?s=%s HTTP/1.1" 200 5 "-" "a" "-" "-"'
    st, rec = e.parse(line % "12x34")
    assert st == OK and rec_value(rec, fields[0]) == "12" and rec_value(rec, fields[1]) == "34"
    st, rec = e.parse(line % "12*34")
    assert st == OK and rec_value(rec, fields[0]) is None and rec_value(rec, fields[1]) is None


@pytest.fixture(scope="module")
def corpus():
    data, lines = rc.corpus()
    a = de.Emu(rc.LOGFORMAT, rc.FIELDS_A, rc.REMAPS, rc.DISSECTORS)
    assert a.status == 0, a.err
    return data, lines, a.parse_batch(data)


def test_corpus_handle_a_is_the_oracles_and_never_fallback(corpus):
    """today's program on the corpus: every line OK, and what the oracle says --
    the condition that keeps the FALLBACK rule of handle B from hiding anything"""
    data, lines, res_a = corpus
    assert len(lines) == 1000 and len(res_a) == 1000
    assert [st for st, _ in res_a] == [OK] * 1000
    o = oracle_lib.Oracle(rc.LOGFORMAT, rc.FIELDS_A, rc.REMAPS)
    for i, line in enumerate(data.decode().split("\n")[:-1]):
        st, js = o.parse_raw(line)
        assert st == oracle_lib.OK, i
        want, got = json.loads(js), res_a[i][1]
        assert got == want, i


def test_corpus_every_line(corpus):
    data, lines, res_a = corpus
    b = de.Emu(rc.LOGFORMAT, rc.FIELDS_B, rc.REMAPS, rc.DISSECTORS)
    assert b.status == 0, b.err
    res_b = b.parse_batch(data)
    n_fb = 0
    for i, ln in enumerate(lines):
        exp = rc.expected(ln)
        st, rec = res_b[i]
        assert st == (FALLBACK if exp is None else OK), (i, ln)
        if exp is None:
            n_fb += 1
            continue
        for f in rc.FIELDS_A:
            assert rec.get(f) == res_a[i][1].get(f), (i, f)
        for f in rc.NEW_FIELDS:
            assert rec_value(rec, f) == exp.get(f), (i, f, ln)
    assert n_fb == rc.planted_fallbacks(lines) and n_fb > 100
    # every category delivered something somewhere
    for f in rc.NEW_FIELDS:
        assert any(rc.expected(ln) and f in rc.expected(ln) for ln in lines), f


def test_corpus_width_only(corpus):
    """the throw depends on what is requested: "1280x" is OK with only the width requested"""
    data, lines, _ = corpus
    fields = rc.FIELDS_A + ["SCREENWIDTH:%s.width" % rc.P_S, "SCREENWIDTH:%s.width" % rc.T_RES]
    w = de.Emu(rc.LOGFORMAT, fields, rc.REMAPS, rc.DISSECTORS)
    res = w.parse_batch(data)
    seen = 0
    for i, ln in enumerate(lines):
        exp = rc.expected(ln, True, False, want_uid=False)  # (no unique-id output: a repeated uid is no cause)
        assert res[i][0] == (FALLBACK if exp is None else OK), (i, ln)
        if exp is not None and rc.expected(ln) is None:
            seen += 1
            for f in fields[len(rc.FIELDS_A):]:
                assert rec_value(res[i][1], f) == exp.get(f), (i, f)
    assert seen > 20


def test_nested_source():
    """a parameter of a derived URI's query (…query.g.query.s): the guard runs after the derived URI stages"""
    data, exp = rc.nested_corpus()
    e = de.Emu(rc.LOGFORMAT, rc.NESTED_FIELDS, rc.NESTED_REMAPS, rc.DISSECTORS)
    assert e.status == 0, e.err
    res = e.parse_batch(data)
    assert len(res) == 64
    for i, (st, rec) in enumerate(res):
        assert st == (FALLBACK if exp[i] is None else OK), i
        if exp[i] is not None:
            for f in rc.NESTED_FIELDS[1:]:
                assert rec_value(rec, f) == exp[i].get(f), (i, f)


def test_reference_restatement_on_the_issue_examples():
    """remap_dissector_ref itself, on the split examples the semantics are stated with"""
    assert ref.screen("x800", True, True) == {"width": "", "height": "800"}
    assert ref.screen("1280x", True, False) == {"width": "1280"}
    assert ref.screen("1x2x3", True, True) == {"width": "1", "height": "2"}
    assert ref.screen("1280X800", True, True) == {} and ref.screen("", True, True) == {} and ref.screen(None, True, True) == {}
    for v in ("1280x", "x", "xx"):
        with pytest.raises(IndexError):
            ref.screen(v, True, True)
    with pytest.raises(IndexError):
        ref.screen("x", True, False)
    assert ref.unique_id("VaGTKApid0AAALpaNo0AAAAC") == {"epoch": 1436652328000, "ip": "10.98.119.64", "processid": 47706,
                                                         "counter": 13965, "threadindex": 2}
    for v in ("Ucdv38CoEJwAAEusp6EAAAD", "Ucdv38CoEJwAAEusp6EAAAD!", "VaGTKApid0A ALpaNo0AAAAC", "VaGTKApid0A=ALpaNo0AAAAC", ""):
        assert ref.unique_id(v) == {}
    assert ref.java_parse_long("+5") == 5 and ref.java_parse_long(" 800") is None and ref.java_parse_long("") is None
    assert ref.java_parse_long("9223372036854775808") is None and ref.java_parse_long("-9223372036854775808") == -(1 << 63)


def test_sanitized_standalone_program():
    """screen_split, unique_id_decode and unique_id_ip (csrc/lp_value.h) against a plain restatement on
    every planted corpus value, at every alignment and at the end of an exactly-sized heap buffer, under
    ASan + UBSan: a program with its own main, run directly"""
    src = os.path.join(ROOT, "tests", "emu", "remapdis_emu.cpp")
    hdr = os.path.join(ROOT, "logparser_amd", "csrc", "lp_value.h")
    prog = os.path.join(BUILD, "remapdis_emu_san")
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(prog) or os.path.getmtime(prog) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        tmp = "%s.%d.tmp" % (prog, os.getpid())
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", tmp, src], check=True)
        os.replace(tmp, prog)
    _, lines = rc.corpus()
    values = sorted({v for ln in lines for v in (ln["s"], ln["uid"], ln["tuid"], ln["tres"]) if v is not None})
    values += [raw for raw, _, _ in rc.SCREEN_PARAM if raw not in (rc.ABSENT, rc.TWICE)]
    values += ["x" * 40, "1x" * 20, "A" * 24, "_" * 24, "-" * 24, "A" * 23 + "\x7f", "9" * 24, "z" * 25]
    assert len(values) > 300
    path = os.path.join(BUILD, "remapdis_emu_input.%d.txt" % os.getpid())
    with open(path, "w") as f:
        f.writelines(v + "\n" for v in values)
    try:
        r = subprocess.run([prog, path], capture_output=True, text=True)
    finally:
        os.remove(path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) == 9 * len(values)
