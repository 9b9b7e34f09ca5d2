"""Corpus and reference of the grouped aggregates (lp_result_group), shared by
test_group_by.py (CPU) and test_group_by_gpu.py.

`reference` is written from the semantics in include/logparser_amd.h, not from
the C: a Python dict in row order over DECODED table values -- None (null),
int (a LONG column's value) or bytes (a STRING column's) -- per row, sums
masked to 64 bits.  On the GPU tests those values are the host copy's table
columns (table_from), which other tests pin against the oracle.

The lines are 'combined' lines with controlled fields; row_select_corpus' BAD
lines and FALLBACK lines (a 0x7F in the user agent) are mixed in."""
import numpy as np

import logparser_amd as lpa
import row_select_corpus as rsc
from where_corpus import BYTES, BYTESCLF, DATE, EPOCH, PATH, QP, STATUS, UA  # noqa: F401 (re-exported)

OK, BAD, FALLBACK = rsc.OK, rsc.BAD, rsc.FALLBACK
METHOD = "HTTP.METHOD:request.firstline.method"
I64_MAX = (1 << 63) - 1
_LINE = b'10.0.%d.%d - u%d [%02d/Oct/%d:13:%02d:%02d +0200] "%s %s HTTP/1.1" %d %s "-" "%s"'
METHODS = (b"GET", b"GET", b"GET", b"POST", b"GET", b"HEAD", b"GET", b"PUT")
STATUSES = (200, 200, 404, 200, 500, 200, 301, 503)


def line(k, method=b"GET", status=200, nbytes=b"100", year=2026, day=None, path=b"/", k7=None, ua=b"curl/8"):
    """one combined line; nbytes: the %b token's text as it is; k7: the query parameter's value (None: absent)"""
    uri = path + (b"?a=%d" % k if k7 is None else b"?a=%d&k7=%s" % (k, k7))
    return _LINE % (k // 256 % 256, k % 256, k, 1 + k % 28 if day is None else day, year, k // 60 % 60, k % 60, method, uri,
                    status, nbytes, ua)


def mixed(n, statuses=True):
    """[(line, status)]: a few methods, statuses, paths and days, bytes "-" / "0" / numbers, the k7 parameter on
    every ninth line; statuses: BAD (k % 5 == 2) and FALLBACK (k % 7 == 4) lines between the OK ones"""
    out = []
    for k in range(n):
        nb = b"-" if k % 5 == 1 else b"0" if k % 5 == 3 else b"%d" % (100 + k % 900)
        l = line(k, METHODS[k % 8], STATUSES[k * 3 % 8], nb, path=b"/p%d" % (k * 7 % 37), k7=b"v%d" % (k % 4) if k % 9 == 0 else None)
        if statuses and k % 5 == 2:
            out.append((rsc.bad_line(k), BAD))
        elif statuses and k % 7 == 4:
            out.append((line(k, ua=b"ua\x7f"), FALLBACK))
        else:
            out.append((l, OK))
    return out


def hot(n):
    """one path on about 90 % of the rows, every other row a path of its own; a hot status as well"""
    return [(line(k, status=200 if k % 10 else 404, nbytes=b"%d" % (k % 1000), path=b"/hot" if k % 10 else b"/only/%d" % k), OK)
            for k in range(n)]


def distinct(n):
    """every row a path of its own"""
    return [(line(k, nbytes=b"%d" % k, path=b"/row/%d" % k), OK) for k in range(n)]


def same(n):
    """every row in one group"""
    return [(line(k, nbytes=b"%d" % (k % 7)), OK) for k in range(n)]


def edges():
    """the value edges: %b "007" and "7" (one LONG group, two STRING groups), "-" and "0" (one BYTES group: CLF2NUM),
    two 9223372036854775807 in one group (the sum wraps), 9223372036854775808 (null as LONG), a group whose measure
    is null on every row, and lines before 1970 (a negative epoch: the minimum)"""
    rows = [(b"/w", b"9223372036854775807", 2026), (b"/z", b"007", 2026), (b"/z", b"7", 2026), (b"/w", b"9223372036854775807", 2026),
            (b"/n", b"-", 2026), (b"/z", b"-", 1969), (b"/z", b"0", 1968), (b"/n", b"9223372036854775808", 2026),
            (b"/w", b"5", 1970), (b"/n", b"-", 1969), (b"/z", b"00", 2026)]
    return [(line(k, nbytes=nb, year=y, path=p), OK) for k, (p, nb, y) in enumerate(rows * 3)]


def words(aggs):
    """accumulator words per group (lpa.group_acc_words): the LDS budget's unit"""
    return lpa.group_acc_words(aggs)


# ------------------------------------------------------------ the reference
def reference(cols, keys, aggs, lines):
    """GROUP BY over rows k = 0 .. len(lines) - 1, row k being batch line lines[k].  cols: {(path, kind): the
    column's decoded value per batch line}.  Returns (rep, group_of, [(value, valid)]): the groups in the order
    of first occurrence, null a key value of its own"""
    groups, rep, group_of, acc = {}, [], [], []
    for i in lines:
        key = tuple(cols[k][i] for k in keys)
        g = groups.setdefault(key, len(rep))
        if g == len(rep):
            rep.append(i)
            acc.append([[] for _ in aggs])
        group_of.append(g)
        for a, cell in zip(aggs, acc[g]):
            v = 1 if a.op == lpa.AGG_COUNT_ROWS else cols[(a.path, int)][i]
            if v is not None:
                cell.append(v)
    fold = {lpa.AGG_COUNT_ROWS: len, lpa.AGG_COUNT: len, lpa.AGG_SUM: lambda c: (sum(c) + (1 << 63)) % (1 << 64) - (1 << 63),
            lpa.AGG_MIN: min, lpa.AGG_MAX: max}
    out = []
    for j, a in enumerate(aggs):
        valid = [a.op <= lpa.AGG_COUNT or len(acc[g][j]) > 0 for g in range(len(rep))]
        out.append((np.array([fold[a.op](acc[g][j]) if valid[g] else 0 for g in range(len(rep))], dtype=np.int64),
                    np.array(valid, dtype=np.uint8)))
    return np.array(rep, dtype=np.int64), np.array(group_of, dtype=np.int32), out
