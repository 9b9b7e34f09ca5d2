"""Predicate row selection, CPU part: the reference evaluator of where_corpus
on hand-built arrays (every op, each negated; nulls; empty operands and empty
values; BETWEEN with lo > hi; the group fold), the entry point's presence and
its null-handle code, and the argument errors of logparser_amd.Where, raised
before any engine call.  The GPU part is test_select_where_gpu.py; the term
rules' C (csrc/lp_pred.h) runs under the sanitizers in
test_select_where_sanitizers.py."""
import ctypes

import numpy as np
import pytest

import logparser_amd as lpa
import row_select_corpus as rsc
import where_corpus as wc
from test_capi import declared_symbols

W = lpa.Where
L, S = ("L", int), ("S", str)
LONGS = [None, -5, 0, 499, 500, 599, 600, 2 ** 63 - 1, -2 ** 63]
STRS = [None, b"", b"/api/x", b"/apix", b"x/api/", b"bot", b"a bot", b"bo", b"&a=1"]


def _rows(col, values, terms, status=None, mask=lpa.SEL_OK, first=0, count=None):
    n = len(values)
    status = np.zeros(n, dtype=np.uint8) if status is None else status
    table = {col: values}
    return wc.expected_rows(table, status, first, n - first if count is None else count, mask, terms).tolist()


def test_reference_long_ops():
    v = LONGS
    idx = lambda pred: [i for i, x in enumerate(v) if pred(x)]  # noqa: E731
    nn = lambda f: (lambda x: x is not None and f(x))  # noqa: E731
    cases = [(lpa.WHERE_EQ, 500, None, nn(lambda x: x == 500)), (lpa.WHERE_LT, 500, None, nn(lambda x: x < 500)),
             (lpa.WHERE_LE, 500, None, nn(lambda x: x <= 500)), (lpa.WHERE_GT, 500, None, nn(lambda x: x > 500)),
             (lpa.WHERE_GE, 500, None, nn(lambda x: x >= 500)),
             (lpa.WHERE_BETWEEN, 500, 599, nn(lambda x: 500 <= x <= 599)),
             (lpa.WHERE_BETWEEN, 599, 500, lambda x: False),  # lo > hi matches nothing
             (lpa.WHERE_BETWEEN, -2 ** 63, 2 ** 63 - 1, nn(lambda x: True))]
    for op, lo, hi, pred in cases:
        assert _rows(L, v, [W("L", op, lo, hi)]) == idx(pred), (op, lo, hi)
        # negated: true on null too (two-valued logic)
        assert _rows(L, v, [W("L", op, lo, hi, negate=True)]) == idx(lambda x: not pred(x)), (op, lo, hi, "negated")
    assert _rows(L, v, [W("L", lpa.WHERE_IS_NULL, kind=int)]) == [0]
    assert _rows(L, v, [W("L", lpa.WHERE_IS_NULL, kind=int, negate=True)]) == list(range(1, len(v)))


def test_reference_string_ops():
    v = STRS
    idx = lambda pred: [i for i, x in enumerate(v) if pred(x)]  # noqa: E731
    nn = lambda f: (lambda x: x is not None and f(x))  # noqa: E731
    cases = [(lpa.WHERE_EQ, b"bot", nn(lambda x: x == b"bot")), (lpa.WHERE_PREFIX, b"/api/", nn(lambda x: x[:5] == b"/api/")),
             (lpa.WHERE_SUFFIX, b"/api/", nn(lambda x: x[-5:] == b"/api/")),
             (lpa.WHERE_CONTAINS, b"bot", nn(lambda x: x.find(b"bot") >= 0)),
             (lpa.WHERE_CONTAINS, b"&", nn(lambda x: b"&" in x)),
             # an empty operand: PREFIX / SUFFIX / CONTAINS on every non-null value, EQ on the empty string only
             (lpa.WHERE_EQ, b"", nn(lambda x: x == b"")), (lpa.WHERE_PREFIX, b"", nn(lambda x: True)),
             (lpa.WHERE_SUFFIX, b"", nn(lambda x: True)), (lpa.WHERE_CONTAINS, b"", nn(lambda x: True)),
             (lpa.WHERE_PREFIX, b"/api/x/longer", lambda x: False)]  # an operand longer than every value
    for op, o, pred in cases:
        assert _rows(S, v, [W("S", op, o)]) == idx(pred), (op, o)
        assert _rows(S, v, [W("S", op, o, negate=True)]) == idx(lambda x: not pred(x)), (op, o, "negated")
    assert _rows(S, v, [W("S", lpa.WHERE_IS_NULL, kind=str)]) == [0]  # an empty string is not null
    assert _rows(S, v, [W("S", lpa.WHERE_IS_NULL, kind=str, negate=True)]) == list(range(1, len(v)))
    assert _rows(S, v, [W("S", lpa.WHERE_EQ, "bot")]) == [5]  # a str operand is its UTF-8 bytes


def test_reference_sql_not_equal():
    """SQL's <> (false on null): EQ | NEGATE and-ed with IS_NULL | NEGATE"""
    terms = [W("S", lpa.WHERE_EQ, b"bot", negate=True, group=0), W("S", lpa.WHERE_IS_NULL, kind=str, negate=True, group=1)]
    assert _rows(S, STRS, terms) == [i for i, x in enumerate(STRS) if x is not None and x != b"bot"]


def test_reference_fold():
    n = 64
    table = {L: [k % 10 if k % 7 else None for k in range(n)], S: [b"p%d" % (k % 4) if k % 5 else None for k in range(n)]}
    st = np.zeros(n, dtype=np.uint8)
    run = lambda terms: wc.expected_rows(table, st, 0, n, 1, terms).tolist()  # noqa: E731
    lv, sv = table[L], table[S]
    # one group: OR
    got = run([W("L", lpa.WHERE_EQ, 3), W("L", lpa.WHERE_EQ, 5), W("S", lpa.WHERE_EQ, b"p1")])
    assert got == [k for k in range(n) if lv[k] in (3, 5) or sv[k] == b"p1"]
    # several groups: AND of ORs; the group numbers need not be consecutive
    got = run([W("L", lpa.WHERE_EQ, 3, group=0), W("L", lpa.WHERE_EQ, 5, group=0), W("S", lpa.WHERE_PREFIX, b"p", group=2),
               W("S", lpa.WHERE_CONTAINS, b"1", group=5, negate=True)])
    assert got == [k for k in range(n) if lv[k] in (3, 5) and sv[k] is not None and not (b"1" in sv[k])]
    # a group that fails early decides every line
    assert run([W("L", lpa.WHERE_LT, -1, group=0), W("S", lpa.WHERE_IS_NULL, kind=str, group=1, negate=True)]) == []
    # eight single-term groups
    got = run([W("L", lpa.WHERE_GE, g, group=g) for g in range(8)])
    assert got == [k for k in range(n) if lv[k] is not None and lv[k] >= 7]


def test_reference_without_terms_is_the_status_select():
    st = np.array([s for _, s in rsc.planted()], dtype=np.uint8)
    for mask in range(8):
        for first, count in ((0, len(st)), (3, 70), (64, 0), (199, 1)):
            assert wc.expected_rows({}, st, first, count, mask, []).tobytes() == \
                rsc.expected_rows(st, first, count, mask).tobytes(), (mask, first, count)


def test_reference_status_and_window():
    st = np.array([0, 1, 2, 0, 0, 2, 1, 0], dtype=np.uint8)
    vals = [b"x", None, None, b"y", None, None, None, b"x"]
    null = [W("S", lpa.WHERE_IS_NULL, kind=str)]
    assert _rows(S, vals, null, status=st, mask=7) == [1, 2, 4, 5, 6]
    assert _rows(S, vals, null, status=st, mask=lpa.SEL_BAD) == [1, 6]
    assert _rows(S, vals, null, status=st, mask=lpa.SEL_OK) == [4]
    assert _rows(S, vals, [W("S", lpa.WHERE_EQ, b"x")], status=st, mask=7, first=1, count=6) == []
    assert _rows(S, vals, [W("S", lpa.WHERE_EQ, b"x")], status=st, mask=7, first=1, count=7) == [7]


def test_corpus_fields():
    """the controlled fields are all there within the first lines"""
    f = [wc.field(k) for k in range(120)]
    assert {x["status"] for x in f} == set(wc.STATUSES)
    assert {None, 0} < {x["bytes"] for x in f} and None in {x["referer"] for x in f}
    assert {len(x["k7"]) for x in f} == {0, 1, 2} and any(x["k7"] == [b""] for x in f)
    assert any(x["ua"].startswith(wc.MARK) for x in f) and any(x["ua"].endswith(wc.MARK) for x in f)
    assert all(any(x["path"].startswith(p) for x in f) for p in wc.PREFIXES)
    mixed = wc.lines(70, "mixed")
    assert {s for _, s in mixed} == {0, 1, 2} and all(b"\n" not in l for l, _ in mixed)
    assert len(wc.with_planted(10)) == 210


# ----------------------------------------------------------- the entry point
def test_entry_point_declared_and_null_handle():
    assert "lp_result_select_where" in declared_symbols()
    lib = lpa.lib()
    n = ctypes.c_uint64(7)
    res = lpa.LpResult()
    assert lib.lp_result_select_where(None, ctypes.byref(res), 0, 0, 1, None, 0, None, 0, ctypes.byref(n)) == lpa.LP_E_INVALID
    assert lib.lp_result_select_where(None, None, 0, 0, 1, None, 0, None, 0, None) == lpa.LP_E_INVALID
    assert ctypes.sizeof(lpa.LpWhereTerm) == 48  # lp_where_term: a pointer, four int32, two int64, a pointer


def test_where_kind_defaults():
    assert W("a:b", lpa.WHERE_GE, 500).kind is int
    assert W("a:b", lpa.WHERE_EQ, "x").kind is str and W("a:b", lpa.WHERE_EQ, "x").value == b"x"
    assert W("a:b", lpa.WHERE_EQ, b"\xff\x00").value == b"\xff\x00"
    assert W("a:b", lpa.WHERE_EQ, "é").value == "é".encode("utf-8")
    assert W("a:b", lpa.WHERE_IS_NULL, kind=int).kind is int and W("a:b", lpa.WHERE_IS_NULL, kind=str, negate=True).negate
    assert W("a:b", lpa.WHERE_BETWEEN, 1, 2).hi == 2
    assert W("a:b", lpa.WHERE_EQ, 5, kind=int, group=3).group == 3


class _NoEngine:
    """a BatchResult stand-in whose engine must never be reached"""
    n_lines = 4
    _select_where = lpa.BatchResult._select_where

    def __getattr__(self, name):
        raise AssertionError("engine reached: " + name)


def test_where_argument_errors_before_any_engine_call():
    bad = [lambda: W("a:b", lpa.WHERE_IS_NULL),                      # kind is required
           lambda: W("a:b", lpa.WHERE_IS_NULL, 5),                   # ... and no operand
           lambda: W("a:b", 10, 5), lambda: W("a:b", -1, 5),         # unknown ops
           lambda: W("a:b", lpa.WHERE_PREFIX, 5),                    # no such op for BIGINT
           lambda: W("a:b", lpa.WHERE_GE, "x"),                      # ... for STRING
           lambda: W("a:b", lpa.WHERE_GE, 5, kind=str),
           lambda: W("a:b", lpa.WHERE_EQ, "x", kind=int),
           lambda: W("a:b", lpa.WHERE_EQ, 5, kind=float),
           lambda: W("a:b", lpa.WHERE_BETWEEN, 5),                   # hi missing
           lambda: W("a:b", lpa.WHERE_GE, 5, 6),                     # hi without BETWEEN
           lambda: W("a:b", lpa.WHERE_GE, 2 ** 63),                  # outside int64
           lambda: W("a:b", lpa.WHERE_CONTAINS, b"x" * 256),         # operand too long
           lambda: W("", lpa.WHERE_GE, 5), lambda: W(None, lpa.WHERE_GE, 5),
           lambda: W("a:b", lpa.WHERE_GE, 5, group=-1),
           lambda: W("a:b", lpa.WHERE_EQ, 1.5)]
    for make in bad:
        with pytest.raises((ValueError, TypeError)):
            make()
    assert W("a:b", lpa.WHERE_CONTAINS, b"x" * 255).value == b"x" * 255
    r = _NoEngine()
    nine = [W("a:b", lpa.WHERE_GE, k) for k in range(9)]
    for terms in (nine, [W("a:b", lpa.WHERE_GE, 1, group=1), W("a:b", lpa.WHERE_GE, 1, group=0)], ["a:b >= 1"]):
        for call in (lambda: lpa.BatchResult.select_where_from(r, lpa.LpResult(), terms),
                     lambda: lpa.BatchResult._select_where(r, lpa.LpResult(), terms, 1, 0, None, None, None)):
            with pytest.raises((ValueError, TypeError)):
                call()
