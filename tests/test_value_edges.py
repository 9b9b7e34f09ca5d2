"""Value edges of the time fields and the typed-table conversions, CPU part
(value_edge_corpus.py: dates before 1970, non-leap centuries, the ends of the
admitted range, Long.parseLong around 2^63 and with signs, seconds-with-millis
values that wrap, Double.parseDouble ties at 2^53..2^59, binary IPs of signed
bytes).  The expectations are the corpus' own (datetime / calendar / int /
float); here the oracle and the CPU emulation of the device per-line code
are compared with them field by field, which pins the corpus itself,
logparser_amd.setters.Value's conversions too, and the pure functions of the
device table (csrc/lp_value.h) run in a stand-alone program under ASan +
UBSan against the C library.  The GPU part is test_value_edges_gpu.py.

A line whose local or UTC year is 10000 has no expectation: the oracle
answers it (status OK, a five-digit year), the device code sends it to
FALLBACK (the reference's rendering of a five-digit year, DateTimeFormatter
"yyyy" with SignStyle.EXCEEDS_PAD, is not restated by the engine)."""
import json
import os
import re
import struct
import subprocess

import pytest

import value_edge_corpus as vc
from logparser_amd.setters import Value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "value_emu.cpp")
CORE_HDR = os.path.join(ROOT, "logparser_amd", "csrc", "lp_value.h")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
OK, BAD, FALLBACK = 0, 1, 2


def _last(rec, path):
    """the value a record's path ends with (the last delivery wins): None | str | int"""
    v = rec.get(path, [None])[-1]
    return v["l"] if isinstance(v, dict) else v


def _time_paths():
    return [p for p, _, _ in vc.TIME_FIELDS]


def _check_time(parser, layout, y10k_status):
    """every line of the layout's corpus through parser.parse_raw: the lines with an expectation OK
    with every field equal, the year-10000 lines with a status of y10k_status"""
    _, lines, exp, none, _ = vc.time_corpus(layout)
    none = set(none)
    for k, line in enumerate(lines):
        st, js = parser.parse_raw(line)
        if k in none:
            assert st in y10k_status, (layout, k, line, st)
            continue
        assert st == OK, (layout, k, line, st)
        rec = json.loads(js)
        for path, _, key in vc.TIME_FIELDS:
            assert _last(rec, path) == exp[k][key], (layout, k, line, path, _last(rec, path), exp[k][key])


@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_time_corpus_sets(layout):
    """the lines without an expectation (outside datetime.date) are exactly the lines whose local or
    UTC year is 10000: 13 of 14 144 in the three date-time layouts, the last of the 7 %s inputs"""
    _, lines, exp, none, y10k = vc.time_corpus(layout)
    assert none == y10k
    assert (len(lines), len(none)) == ((7, 1) if layout == "epoch" else (14144, 13))
    assert len(set(lines)) == len(lines)
    # the corpus reaches what it is for
    if layout != "epoch":
        years = {e["year_utc"] for e in exp if e} | {e["year"] for e in exp if e}
        assert {999, 1000, 1899, 1900, 1969, 1970, 2100, 9999} <= years
        assert min(e["epoch"] for e in exp if e) < 0
        assert {52, 53, 1} <= {e["weekofweekyear"] for e in exp if e}


@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_time_oracle(oracle, layout):
    """the oracle's calendar against datetime; it answers the year-10000 lines its own way (OK with a
    five-digit year, or -- its strftime resolver past year 9999 -- UNSUPPORTED)"""
    _check_time(oracle.Oracle(vc.FORMATS[layout], _time_paths()), layout, (OK, oracle.UNSUPPORTED))


@pytest.mark.parametrize("layout", vc.LAYOUTS)
def test_time_emu(emu, layout):
    """the device per-line code's calendar (lp_device.h on the CPU) against datetime; the
    year-10000 lines are FALLBACK in every layout"""
    e = emu.Emu(vc.FORMATS[layout], _time_paths())
    assert e.status == 0, e.err
    _check_time(e, layout, (FALLBACK,))


def _check_numbers(parser):
    lines, exp = vc.number_corpus()
    paths = vc.num_paths()
    for k, line in enumerate(lines):
        st, js = parser.parse_raw(line)
        if exp[k] is None:
            assert st == BAD, (k, line, st)
            continue
        assert st == OK, (k, line, st)
        rec = json.loads(js)
        for path in paths:
            assert _last(rec, path) == exp[k][path], (k, line, path, _last(rec, path), exp[k][path])


def test_number_corpus_shape():
    """what the corpus is for is in it, and mixed: every 64 consecutive rows hold a 1-character
    and a 20-character long, a negative one, a null and a BAD line"""
    lines, exp = vc.number_corpus()
    ms = "MILLISECONDS:response.server.processing.time"
    for k0 in range(0, len(lines) - 64):
        w = exp[k0:k0 + 64]
        vals = [e[ms] for e in w if e]
        assert any(e is None for e in w) and 0 in vals and -(1 << 63) in vals and any(v < 0 for v in vals), k0
        assert any(e and e["PORT:nginxmodule.realip.remote_port"] is None for e in w), k0
    texts = set(vc.decimal_strings())
    assert {"999999999999999999.999", "9007199254740993.0", "0.000000000000000001", "4503599627370497.5"} <= texts
    assert all(len(i) <= 18 and len(f) <= 18 for i, f in (t.split(".") for t in texts))
    # each signed byte in each position of the binary address
    seen = {(j, int(b)) for e in exp if e for j, b in enumerate(re.findall(r"-?[0-9]+", e["IP:connection.client.host"]))}
    assert seen >= {(j, b) for j in range(4) for b in vc.BIN_BYTES}


def test_numbers_oracle(oracle):
    _check_numbers(oracle.Oracle(vc.NUM_FMT, vc.num_paths()))


def test_numbers_emu(emu):
    e = emu.Emu(vc.NUM_FMT, vc.num_paths())
    assert e.status == 0, e.err
    _check_numbers(e)


def test_signed_long_source(emu):
    """whether a LONG-cast token admits a sign: of the corpus' tokens only $realip_remote_port (the
    planner's casts say STRING | LONG, and "-5" is delivered as written)"""
    import logparser_amd as lpa
    e = emu.Emu(vc.NUM_FMT, vc.num_paths())
    assert e.casts("PORT:nginxmodule.realip.remote_port") == lpa.CAST_STRING | lpa.CAST_LONG
    assert e.casts("BYTES:response.body.bytes") == lpa.CAST_STRING | lpa.CAST_LONG
    assert e.casts("SECOND_MILLIS:nginxmodule.upstream.response.time.0.value") & lpa.CAST_DOUBLE
    st, rec = e.parse(b'5 0.1 "0.1" \\x00\\x00\\x00\\x00 [-5]')
    assert st == OK and rec["PORT:nginxmodule.realip.remote_port"] == ["-5"]
    st, _ = e.parse(b'-5 0.1 "0.1" \\x00\\x00\\x00\\x00 [5]')  # $body_bytes_sent: [0-9]+
    assert st == BAD


def test_setters_value_conversions():
    """Value.get_long / get_double (the host side's Long.parseLong / Double.parseDouble) on the corpus' texts"""
    for t in vc.BYTES + vc.PORTS:
        assert Value(t).get_long() == vc.java_long(t), t
    assert Value("9223372036854775807").get_long() == (1 << 63) - 1 and Value("9223372036854775808").get_long() is None
    assert Value("-9223372036854775808").get_long() == -(1 << 63) and Value("+5").get_long() == 5
    for t in vc.decimal_strings():
        got = Value(t).get_double()
        assert struct.pack("<d", got) == struct.pack("<d", float(t)), t
        ms = vc.secms(t)
        assert Value(ms).get_string() == str(ms) and Value(ms).get_long() == ms
        assert struct.pack("<d", Value(ms).get_double()) == struct.pack("<d", float(ms)), t


def _build(target, flags):
    os.makedirs(BUILD, exist_ok=True)
    if os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(EMU_SRC), os.path.getmtime(CORE_HDR)):
        return target
    tmp = "%s.%d.tmp" % (target, os.getpid())  # renamed into place: parallel workers never see half a file
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-o", tmp] + flags + [EMU_SRC], check=True)
    os.replace(tmp, target)
    return target


def test_sanitized_standalone_program():
    """digits, write_long, parse_long and decimal_to_double (csrc/lp_value.h, the header the table
    kernels include) against snprintf / strtoll / strtod on the corpus' values and a few million
    random ones, under ASan + UBSan: a program with its own main, run directly"""
    prog = _build(os.path.join(BUILD, "value_emu_san"), ASAN)
    _, exp = vc.number_corpus()
    longs = sorted({v for e in exp if e for v in e.values() if isinstance(v, int)})
    path = os.path.join(BUILD, "value_emu_input.%d.txt" % os.getpid())
    with open(path, "w") as f:
        f.writelines("D %s\n" % t for t in vc.decimal_strings())
        f.writelines("L %s\n" % t for t in vc.BYTES + vc.PORTS if t and "\n" not in t)
        f.writelines("W %d\n" % v for v in longs)
    try:
        r = subprocess.run([prog, path], capture_output=True, text=True)
    finally:
        os.remove(path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "total: 0 differ" in r.stdout, r.stdout
    n_l = len([t for t in vc.BYTES + vc.PORTS if t])
    assert "file: %d decimals, %d texts, %d longs" % (len(vc.decimal_strings()), n_l, len(longs)) in r.stdout, r.stdout
    for name in ("decimal_to_double", "parse_long", "digits / write_long"):
        assert name + ":" in r.stdout, r.stdout
