"""Grouped aggregates (lp_result_group), CPU part: the reference of
group_corpus on hand-built arrays (null against "", LONG against STRING
equality, the wrapping sum, all-null measures, no keys, no rows), the argument
errors of logparser_amd.Agg and of the key / aggregate lists, raised before any
engine call, and the entry points' presence, struct layouts and null-handle
code.  The GPU part is test_group_by_gpu.py; the core's C (csrc/lp_group.h)
runs under the sanitizers in test_group_by_sanitizers.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import group_corpus as gc
import logparser_amd as lpa
from test_capi import declared_symbols

A = lpa.Agg
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, CNT, SUM, MIN, MAX = lpa.AGG_COUNT_ROWS, lpa.AGG_COUNT, lpa.AGG_SUM, lpa.AGG_MIN, lpa.AGG_MAX


def _ref(cols, keys, aggs, lines=None):
    n = len(next(iter(cols.values())))
    rep, group_of, out = gc.reference(cols, keys, aggs, range(n) if lines is None else lines)
    return rep.tolist(), group_of.tolist(), [(v.tolist(), ok.tolist()) for v, ok in out]


def test_reference_null_is_a_key_distinct_from_empty():
    cols = {("S", str): [None, b"", b"a", None, b"", b"a", b"b"], ("L", int): [1, 2, 3, 4, 5, 6, 7]}
    rep, group_of, out = _ref(cols, [("S", str)], [A(ROWS), A(SUM, "L")])
    assert rep == [0, 1, 2, 6] and group_of == [0, 1, 2, 0, 1, 2, 3]
    assert out[0] == ([2, 2, 2, 1], [1, 1, 1, 1]) and out[1] == ([5, 7, 9, 7], [1, 1, 1, 1])


def test_reference_long_equality_is_by_value_string_by_bytes():
    # the %b tokens "007", "7", "-", "0": as LONG 7, 7, null, 0; as STRING their bytes (null for "-")
    cols = {("B", int): [7, 7, None, 0], ("B", str): [b"007", b"7", None, b"0"]}
    assert _ref(cols, [("B", int)], [A(ROWS)])[:2] == ([0, 2, 3], [0, 0, 1, 2])
    assert _ref(cols, [("B", str)], [A(ROWS)])[:2] == ([0, 1, 2, 3], [0, 1, 2, 3])


def test_reference_wrap_min_max_and_all_null_measure():
    big = gc.I64_MAX
    cols = {("K", str): [b"w", b"w", b"n", b"n", b"w"], ("L", int): [big, big, None, None, -5]}
    rep, group_of, out = _ref(cols, [("K", str)], [A(SUM, "L"), A(MIN, "L"), A(MAX, "L"), A(CNT, "L"), A(ROWS)])
    assert rep == [0, 2] and group_of == [0, 0, 1, 1, 0]
    assert out[0] == ([(2 * big - 5 + (1 << 63)) % (1 << 64) - (1 << 63), 0], [1, 0])  # two's-complement wrap; no value: valid 0
    assert out[0][0][0] == -7
    assert out[1] == ([-5, 0], [1, 0]) and out[2] == ([big, 0], [1, 0])
    assert out[3] == ([3, 0], [1, 1]) and out[4] == ([3, 2], [1, 1])  # the counts are always valid


def test_reference_no_keys_no_rows_row_lists_and_composites():
    cols = {("K", str): [b"a", b"b", b"a"], ("J", int): [1, 1, 2], ("L", int): [10, 20, 30]}
    assert _ref(cols, [], [A(ROWS), A(SUM, "L")]) == ([0], [0, 0, 0], [([3], [1]), ([60], [1])])
    assert _ref(cols, [], [A(ROWS)], lines=[]) == ([], [], [([], [])])
    assert _ref(cols, [("K", str)], [A(ROWS)], lines=[]) == ([], [], [([], [])])
    # a row list that repeats and runs backwards: the order follows k, rep is the line
    assert _ref(cols, [("K", str)], [A(SUM, "L")], lines=[2, 1, 2, 0]) == ([2, 1], [0, 1, 0, 0], [([70, 20], [1, 1])])
    # a composite in which only the last key differs
    assert _ref(cols, [("K", str), ("J", int)], [A(ROWS)])[:2] == ([0, 1, 2], [0, 1, 2])
    assert _ref(cols, [("J", int), ("K", str)], [A(ROWS)])[:2] == ([0, 1, 2], [0, 1, 2])


def test_acc_words():
    assert lpa.group_acc_words([]) == 1 and lpa.group_acc_words([A(ROWS)]) == 1
    assert lpa.group_acc_words([A(ROWS), A(SUM, "L")]) == 3
    assert lpa.group_acc_words([A(SUM, "L"), A(MIN, "L"), A(MAX, "L"), A(CNT, "L"), A(CNT, "M")]) == 1 + 2 + 3


def test_agg_argument_errors():
    for bad in (lambda: A(5), lambda: A(-1), lambda: A("sum", "L"), lambda: A(True, "L"), lambda: A(ROWS, "L"),
                lambda: A(SUM), lambda: A(SUM, ""), lambda: A(MIN, b"L"), lambda: A(CNT, None)):
        with pytest.raises(ValueError):
            bad()
    assert repr(A(SUM, "L")) == "Agg(2, 'L')" and A(ROWS).path is None
    with pytest.raises(ValueError):
        lpa._group_args([("K", str)] * 5, [])
    with pytest.raises(ValueError):
        lpa._group_args([], [A(ROWS)] * 9)
    with pytest.raises(TypeError):
        lpa._group_args([], [(SUM, "L")])
    for bad_key in ("K", ("K",), ("K", float), ("", str), (b"K", str)):
        with pytest.raises(ValueError):
            lpa._group_args([bad_key], [])
    keys, aggs = lpa._group_args([("K", str), ("J", int)], [A(ROWS), A(MAX, "L")])
    assert (keys[0].path, keys[0].kind, keys[1].kind) == (b"K", lpa.CAST_STRING, lpa.CAST_LONG)
    assert (aggs[0].path, aggs[0].op, aggs[1].path, aggs[1].op) == (None, ROWS, b"L", MAX)
    assert lpa._group_args([], []) == (None, None)


def test_entry_points_and_null_handle():
    assert {"lp_result_group", "lp_result_group_rows"} <= set(declared_symbols())
    L = lpa.lib()
    out, res = lpa.LpGroupOut(), lpa.LpResult()
    assert L.lp_result_group(None, ctypes.byref(res), 0, 0, None, 0, None, 0, ctypes.byref(out), 1) == lpa.LP_E_INVALID
    assert L.lp_result_group_rows(None, ctypes.byref(res), None, 0, None, 0, None, 0, ctypes.byref(out), 1) == lpa.LP_E_INVALID
    assert L.lp_set_option(None, lpa.OPT_GROUP_LDS_WORDS, 0) == lpa.LP_E_INVALID
    assert (lpa.AGG_COUNT_ROWS, lpa.AGG_COUNT, lpa.AGG_SUM, lpa.AGG_MIN, lpa.AGG_MAX) == (0, 1, 2, 3, 4)


def test_struct_layouts_match_the_header(tmp_path):
    """offsetof / sizeof of the three structs as a C compiler sees the header, against the ctypes mirrors"""
    structs = {"lp_group_key": lpa.LpGroupKey, "lp_group_agg": lpa.LpGroupAgg, "lp_group_out": lpa.LpGroupOut}
    src = tmp_path / "layout.c"
    body = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % os.path.join(ROOT, "include", "logparser_amd.h"),
            "int main(void) {"]
    want = []
    for name, cls in structs.items():
        for f, _ in cls._fields_:
            body.append('  printf("%%zu ", offsetof(%s, %s));' % (name, f))
            want.append(getattr(cls, f).offset)
        body.append('  printf("%%zu ", sizeof(%s));' % name)
        want.append(ctypes.sizeof(cls))
    body += ['  printf("%d %d\\n", LP_GROUP_MAX_KEYS, LP_GROUP_MAX_AGGS);', "  return 0;", "}"]
    want += [lpa.GROUP_MAX_KEYS, lpa.GROUP_MAX_AGGS]
    src.write_text("\n".join(body) + "\n")
    prog = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(prog), str(src)], check=True)
    got = subprocess.run([str(prog)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == want
    assert np.dtype(np.int64).itemsize == 8
