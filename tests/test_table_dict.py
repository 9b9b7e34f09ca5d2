"""Dictionary-encoded STRING columns (lp_result_table_dict,
lp_result_table_dict_rows), CPU part: dict_corpus.expected_dict and
logparser_amd.strings_from_dict on hand-built arrays, the C ABI's new entry
points and the struct's layout, and the stand-alone program of the host-
compilable core (tests/emu/dict_emu.cpp over csrc/lp_dict.h) under ASan + UBSan
and, where its runtime exists, ThreadSanitizer.  The GPU part is
test_table_dict_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np

import dict_corpus as dc
import logparser_amd as lpa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "dict_emu.cpp")
CORE_HDR = os.path.join(ROOT, "logparser_amd", "csrc", "lp_dict.h")
HEADER = os.path.join(ROOT, "include", "logparser_amd.h")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
TSAN = ["-fsanitize=thread", "-fno-omit-frame-pointer"]


def _arrow(values):
    """a plain Arrow STRING column of bytes | None values"""
    off = np.zeros(len(values) + 1, dtype=np.int64)
    np.cumsum([len(v or b"") for v in values], out=off[1:])
    chars = np.frombuffer(b"".join(v or b"" for v in values), dtype=np.uint8)
    return off, chars, np.array([v is not None for v in values], dtype=np.uint8)


def test_expected_dict():
    # null rows, "" against null, a prefix of another value, values differing in the last byte only
    vals = [None, b"ab", b"", None, b"abc", b"ab", b"abd", b"", b"abc", None]
    idx, off, chars = dc.expected_dict(*_arrow(vals))
    assert idx.dtype == np.int32 and off.dtype == np.int64 and chars.dtype == np.uint8
    assert idx.tolist() == [0, 0, 1, 0, 2, 0, 3, 1, 2, 0]
    assert off.tolist() == [0, 2, 2, 5, 8] and chars.tobytes() == b"ababcabd"
    idx, off, chars = dc.expected_dict(*_arrow([None, None]))
    assert idx.tolist() == [0, 0] and off.tolist() == [0] and chars.size == 0
    idx, off, chars = dc.expected_dict(*_arrow([]))
    assert idx.size == 0 and off.tolist() == [0]
    idx, off, chars = dc.expected_dict(*_arrow([b"", b""]))  # "" is a value and gets an entry
    assert idx.tolist() == [0, 0] and off.tolist() == [0, 0]
    # first occurrence, not sorted order
    idx, off, chars = dc.expected_dict(*_arrow([b"z", b"a", b"z", b"m"]))
    assert idx.tolist() == [0, 1, 0, 2] and chars.tobytes() == b"zam"


def test_strings_from_dict():
    vals = [None, b"ab", b"", None, b"abc", b"ab", "été".encode(), b""]
    off, chars, valid = _arrow(vals)
    idx, doff, dchars = dc.expected_dict(off, chars, valid)
    got = lpa.strings_from_dict(valid, idx, doff, dchars)
    assert got == [None if v is None else v.decode("utf-8") for v in vals]
    assert lpa.strings_from_dict([], [], [0], b"") == []
    assert lpa.strings_from_dict([0, 0], [0, 0], [0], b"") == [None, None]


def test_corpus_lines():
    """the corpus' paths are paths of the format; a common line is the combined line's head"""
    paths = set(lpa.get_possible_paths(dc.FMT))
    for p in (dc.UA, dc.PATH, dc.QUERY, dc.STATUS, dc.BYTES, dc.DATE, dc.MONTHNAME, dc.METHOD, dc.REFERER, dc.REQ):
        assert p in paths, p
    common = set(lpa.get_possible_paths("common"))
    assert all(p in common for p in dc.COMMON_FIELDS) and dc.UA not in common
    assert dc.line(5).startswith(dc.common_line(5) + b' "') and dc.common_line(5).endswith(b" 301 5000")


def test_abi_entry_points_and_layout():
    """the library exports the two calls (without a handle each is
    LP_E_INVALID), the header declares them, the option has its number and the
    ctypes mirror of lp_table_dict_col has the C struct's layout"""
    L = lpa.lib()
    res = lpa.LpResult()
    col = lpa.LpTableDictCol()
    assert L.lp_result_table_dict(None, ctypes.byref(res), 0, 0, ctypes.byref(col), 1, 1) == lpa.LP_E_INVALID
    assert L.lp_result_table_dict_rows(None, ctypes.byref(res), None, 0, ctypes.byref(col), 1, 1) == lpa.LP_E_INVALID
    from test_capi import declared_symbols
    assert {"lp_result_table_dict", "lp_result_table_dict_rows"} <= set(declared_symbols())
    with open(HEADER) as f:
        src = f.read()
    assert int(re.search(r"#define LP_OPT_DICT_HASH_BITS (\d+)", src).group(1)) == lpa.OPT_DICT_HASH_BITS
    fields = ["path", "valid", "index", "dict_off", "dict_chars", "dict_cap", "dict_chars_cap", "dict_len", "dict_chars_len"]
    assert [f[0] for f in lpa.LpTableDictCol._fields_] == fields
    os.makedirs(BUILD, exist_ok=True)
    prog = os.path.join(BUILD, "dict_layout")
    csrc = prog + ".%d.c" % os.getpid()
    with open(csrc, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n' % HEADER)
        for name in fields:
            f.write('  printf("%%zu ", offsetof(lp_table_dict_col, %s));\n' % name)
        f.write('  printf("%zu\\n", sizeof(lp_table_dict_col));\n  return 0;\n}\n')
    tmp = "%s.%d.tmp" % (prog, os.getpid())
    subprocess.run(["gcc", "-std=c99", "-o", tmp, csrc], check=True)
    os.replace(tmp, prog)
    os.remove(csrc)
    out = subprocess.run([prog], capture_output=True, text=True, check=True).stdout.split()
    want = [getattr(lpa.LpTableDictCol, name).offset for name in fields] + [ctypes.sizeof(lpa.LpTableDictCol)]
    assert [int(x) for x in out] == want, (out, want)


def _build(target, flags):
    os.makedirs(BUILD, exist_ok=True)
    if os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(EMU_SRC), os.path.getmtime(CORE_HDR)):
        return target
    tmp = "%s.%d.tmp" % (target, os.getpid())  # renamed into place: parallel workers never see half a file
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-pthread", "-o", tmp] + flags + [EMU_SRC], check=True)
    os.replace(tmp, target)
    return target


def _run_emu(prog):
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "total: 0 differ" in r.stdout and "full table: reported" in r.stdout, r.stdout
    for bits in (0, 1, 2):
        for threads in (1, 4, 7):
            assert "bits %d threads %d:" % (bits, threads) in r.stdout, r.stdout


def test_sanitized_standalone_program():
    """the adversarial value set through the host build of the hash and the
    insert, single-threaded and from several threads, the hash whole and
    narrowed to 1 and 2 bits, under ASan + UBSan: a program with its own main,
    run directly"""
    _run_emu(_build(os.path.join(BUILD, "dict_emu_san"), ASAN))


def test_thread_sanitized_standalone_program():
    """the same program under ThreadSanitizer (the build machine has its runtime)"""
    _run_emu(_build(os.path.join(BUILD, "dict_emu_tsan"), TSAN))
