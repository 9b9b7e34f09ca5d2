"""Row selection (lp_result_select, lp_result_table_rows,
lp_result_table_map_rows, the pseudo-columns), CPU part: the helpers of
row_select_corpus on hand-built arrays, every planted status confirmed (OK /
BAD by the oracle, FALLBACK by the emulation of the device per-line code, as
test_uri_wave.py does for its corpora), and the C ABI's new entry points.  The
GPU part is test_row_select_gpu.py."""
import ctypes
import os
import re

import numpy as np

import corpora
import logparser_amd as lpa
import row_select_corpus as rsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_expected_rows():
    st = np.array([0, 1, 2, 0, 0, 2, 1, 0], dtype=np.uint8)
    assert rsc.expected_rows(st, 0, 8, lpa.SEL_OK).tolist() == [0, 3, 4, 7]
    assert rsc.expected_rows(st, 0, 8, lpa.SEL_BAD | lpa.SEL_FALLBACK).tolist() == [1, 2, 5, 6]
    assert rsc.expected_rows(st, 2, 4, lpa.SEL_FALLBACK).tolist() == [2, 5]  # batch-relative, not window-relative
    assert rsc.expected_rows(st, 3, 0, 7).tolist() == [] and rsc.expected_rows(st, 0, 8, 0).tolist() == []
    assert rsc.expected_rows(st, 0, 8, 7).tolist() == list(range(8))
    assert rsc.expected_rows(st, 0, 8, 7).dtype == np.int64
    assert (lpa.SEL_OK, lpa.SEL_BAD, lpa.SEL_FALLBACK) == (1, 2, 4)


def test_gather_arrow():
    off = np.array([0, 2, 2, 5, 6], dtype=np.int64)
    chars = np.frombuffer(b"abcdef", dtype=np.uint8)
    valid = np.array([1, 0, 1, 1], dtype=np.uint8)
    o, c, v = rsc.gather_arrow(off, chars, valid, [3, 0, 0, 1, 2])
    assert o.tolist() == [0, 1, 3, 5, 5, 8] and c.tobytes() == b"fababcde" and v.tolist() == [1, 1, 1, 0, 1]
    o, c, v = rsc.gather_arrow(off, chars, valid, [])
    assert o.tolist() == [0] and c.size == 0 and v.size == 0
    o, c, v = rsc.gather_arrow(off, chars, valid, range(4))
    assert o.tolist() == off.tolist() and c.tobytes() == b"abcdef" and v.tolist() == valid.tolist()


def test_gather_map():
    whole = {"valid": np.array([1, 0, 1], np.uint8), "entry_off": np.array([0, 2, 2, 3], np.int64),
             "key_off": np.array([0, 1, 3, 6], np.int64), "key_chars": np.frombuffer(b"abbccc", np.uint8),
             "val_off": np.array([0, 0, 1, 3], np.int64), "val_chars": np.frombuffer(b"xyz", np.uint8)}
    g = rsc.gather_map(whole, [2, 0, 2, 1])
    assert g["valid"].tolist() == [1, 1, 1, 0] and g["entry_off"].tolist() == [0, 1, 3, 4, 4]
    assert g["key_off"].tolist() == [0, 3, 4, 6, 9] and g["key_chars"].tobytes() == b"cccabbccc"
    assert g["val_off"].tolist() == [0, 2, 2, 3, 5] and g["val_chars"].tobytes() == b"yzxyz"
    assert lpa.maps_from_arrow(*(g[n] for n in lpa.MAP_ARRAYS)) == [{"ccc": "yz"}, {"a": "", "bb": "x"}, {"ccc": "yz"}, None]
    g = rsc.gather_map(whole, [])
    assert [g[n].tolist() for n in lpa.MAP_ARRAYS] == [[], [0], [0], [], [0], []]
    # a window is a gather of consecutive rows (test_table_map_gpu._window_of)
    g = rsc.gather_map(whole, [1, 2])
    assert g["entry_off"].tolist() == [0, 0, 1] and g["key_chars"].tobytes() == b"ccc" and g["val_off"].tolist() == [0, 2]


def test_planted_statuses(oracle, emu):
    """every planted status is what the oracle (OK / BAD) and the device
    per-line code (FALLBACK) say of the line"""
    fields = oracle.possible_paths(rsc.FMT)
    o = oracle.Oracle(rsc.FMT, fields)
    e = emu.Emu(rsc.FMT, fields)
    assert e.status == 0, e.err
    seen = set()
    for pattern in (None, "ok", "none", "third", "mixed"):
        lines = rsc.planted() if pattern is None else rsc.pattern_lines(67, pattern)
        for k, (l, st) in enumerate(lines):
            got = e.parse_raw(l)[0]
            assert got == st, (pattern, k, l[:80], got, st)
            if st != rsc.FALLBACK:
                assert o.parse_raw(l)[0] == (oracle.OK if st == rsc.OK else oracle.BAD), (pattern, k, l[:80])
            seen.add(st)
    assert seen == {rsc.OK, rsc.BAD, rsc.FALLBACK}
    lines = [l for l, _ in rsc.planted()]
    assert max(len(l) for l in lines) > 8191 and b"" in lines
    bad_utf8 = 0
    for l in lines:
        try:
            l.decode("utf-8")
        except UnicodeDecodeError:
            bad_utf8 += 1
    assert bad_utf8 == 1


def test_variants_split_back():
    lines = [l for l, _ in rsc.planted()]
    v = rsc.variants(lines)
    assert b"\r\n" in v["crlf"] and not v["crlf"].endswith((b"\n", b"\r")) and not v["unterminated"].endswith(b"\n")
    assert v["lonecr"].count(b"\r") - v["lonecr"].count(b"\r\n") > 50
    for data in v.values():
        assert corpora.split_hadoop(data) == lines


def test_select_tiles_match_the_kernels():
    """SEL_WAVE_LINES / SEL_BLOCK_LINES of the package are the select kernels' tiles (csrc/kernels.h)"""
    with open(os.path.join(ROOT, "logparser_amd", "csrc", "kernels.h")) as f:
        src = f.read()
    w = int(re.search(r"constexpr int SEL_WAVE_LINES = (\d+);", src).group(1))
    b = int(re.search(r"constexpr int SEL_BLOCK_LINES = (\d+);", src).group(1))
    assert (w, b) == (lpa.SEL_WAVE_LINES, lpa.SEL_BLOCK_LINES) and w == 64 * 16 and b % w == 0


def test_new_entry_points_exported():
    """the library exports the three calls; without a handle each is LP_E_INVALID"""
    L = lpa.lib()
    res = lpa.LpResult()
    n = ctypes.c_uint64(99)
    assert L.lp_result_select(None, ctypes.byref(res), 0, 0, lpa.SEL_OK, None, 0, ctypes.byref(n)) == lpa.LP_E_INVALID
    col, mcol = lpa.LpTableCol(), lpa.LpTableMapCol()
    assert L.lp_result_table_rows(None, ctypes.byref(res), None, 0, ctypes.byref(col), 1, 1) == lpa.LP_E_INVALID
    assert L.lp_result_table_map_rows(None, ctypes.byref(res), None, 0, ctypes.byref(mcol), 1, 1) == lpa.LP_E_INVALID
    from test_capi import declared_symbols
    assert {"lp_result_select", "lp_result_table_rows", "lp_result_table_map_rows"} <= set(declared_symbols())


def test_rows_exclude_a_window():
    """rows together with first / count is a ValueError (before any engine call)"""
    import pytest
    r = lpa.BatchResult.__new__(lpa.BatchResult)
    r.n_lines = 4
    rows = np.zeros(2, dtype=np.int64)
    for kw in ({"first": 1}, {"count": 2}):
        with pytest.raises(ValueError):
            r.table_from(None, [("@line", str)], rows=rows, **kw)
        with pytest.raises(ValueError):
            r.table_map_from(None, ["STRING:request.firstline.uri.query.*"], rows=rows, **kw)
    with pytest.raises(ValueError):
        r.table_from(None, [("@line", str)], rows=[0, 1])  # not an int64 array
