"""Corpus and reference evaluator of the predicate row selection
(lp_result_select_where), shared by test_select_where.py (CPU) and
test_select_where_gpu.py.

expected_rows is written from the semantics in include/logparser_amd.h, not
from the C: a dozen lines of Python over DECODED table values -- None (null),
int (a LONG column's value) or bytes (a STRING column's) -- per line of the
batch.

The lines are 'combined' lines with controlled fields (field(k) names what
line k holds), row_select_corpus' BAD and FALLBACK lines mixed in."""
import numpy as np

import logparser_amd as lpa
import row_select_corpus as rsc

OK, BAD, FALLBACK = rsc.OK, rsc.BAD, rsc.FALLBACK

STATUS = "STRING:request.status.last"
BYTESCLF = "BYTESCLF:response.body.bytes"   # the %b token: "-" is null
BYTES = "BYTES:response.body.bytes"         # its converter: "-" is 0
EPOCH = "TIME.EPOCH:request.receive.time.epoch"
DATE = "TIME.DATE:request.receive.time.date"
PATH = "HTTP.PATH:request.firstline.uri.path"
QUERY = "HTTP.QUERYSTRING:request.firstline.uri.query"  # raw: with its leading '&'
QP = "STRING:request.firstline.uri.query.k7"
QWILD = "STRING:request.firstline.uri.query.*"
REFERER = "HTTP.URI:request.referer"
UA = "HTTP.USERAGENT:request.user-agent"
MARK = b"bot"

STATUSES = (200, 404, 500, 502, 503, 301)
PREFIXES = (b"/api/v1/item", b"/static/css/f", b"/p")
_LINE = b'10.0.%d.%d - u%d [%02d/Oct/2026:13:%02d:%02d +0200] "GET %s HTTP/1.1" %d %s "%s" "%s"'


def field(k):
    """what line k holds: status, bytes (None: "-"), referer (None: "-"), path, the k7 parameter's
    occurrences (a list of values: absent [], empty [b""], once, repeated -- the last wins) and the user agent"""
    k7 = ([], [b""], [b"v%d" % k], [b"first", b"w%d" % (k % 5)])[k % 4]
    ua = (b"bot-agent/1.%d" % (k % 3), b"Mozilla/5.0 (X11; k%d)" % k, b"Mozilla crawler %d bot" % k, b"curl/8")[k // 2 % 4]
    return {"status": STATUSES[k % len(STATUSES)], "bytes": None if k % 5 == 1 else 0 if k % 5 == 3 else 100 + k % 900,
            "referer": None if k % 3 == 0 else b"http://h.example.com/r?x=%d" % k,
            "path": PREFIXES[k // 3 % 3] + b"%d" % k, "k7": k7, "ua": ua, "day": 1 + k % 28, "min": k // 60 % 60, "sec": k % 60}


def ok_line(k, ua=None):
    f = field(k)
    query = b"&".join([b"a=%d" % k] + [b"k7=" + v for v in f["k7"]]) if k % 7 else b"&".join(b"k7=" + v for v in f["k7"])
    uri = f["path"] + (b"?" + query if query else b"")
    return _LINE % (k // 256 % 256, k % 256, k, f["day"], f["min"], f["sec"], uri, f["status"],
                    b"-" if f["bytes"] is None else b"%d" % f["bytes"], f["referer"] or b"-", ua or f["ua"])


def common_line(k):
    """line k in the 'common' LogFormat: without the referer and the user agent"""
    l = ok_line(k)
    return l[:l.rindex(b' "', 0, l.rindex(b' "'))]


def lines(n, pattern="ok"):
    """[(line, status)]: n lines; 'ok' all OK, 'mixed' row_select_corpus' BAD (k % 5 == 2) and FALLBACK
    (k % 7 == 4: a 0x7F in the user agent) lines between them, as its pattern_lines"""
    if pattern == "ok":
        return [(ok_line(k), OK) for k in range(n)]
    assert pattern == "mixed"
    return [(rsc.bad_line(k), BAD) if k % 5 == 2 else (ok_line(k, ua=b"ua\x7f" + MARK), FALLBACK) if k % 7 == 4
            else (ok_line(k), OK) for k in range(n)]


def with_planted(n):
    """rsc.planted()'s 200 lines (the line longer than 8191 bytes, the invalid UTF-8, the empty line) after n of ours"""
    return lines(n, "mixed") + rsc.planted()


# ------------------------------------------------------------ the reference
def term_holds(term, v):
    """one term (a logparser_amd.Where) on one decoded value: two-valued -- a comparison with null is
    false, IS_NULL is true exactly on null, negate flips the outcome after that"""
    if term.op == lpa.WHERE_IS_NULL:
        r = v is None
    elif v is None:
        r = False
    elif term.kind is int:
        r = {lpa.WHERE_EQ: v == term.value, lpa.WHERE_LT: v < term.value, lpa.WHERE_LE: v <= term.value,
             lpa.WHERE_GT: v > term.value, lpa.WHERE_GE: v >= term.value,
             lpa.WHERE_BETWEEN: term.hi is not None and term.value <= v <= term.hi}[term.op]
    else:
        r = {lpa.WHERE_EQ: v == term.value, lpa.WHERE_PREFIX: v.startswith(term.value),
             lpa.WHERE_SUFFIX: v.endswith(term.value), lpa.WHERE_CONTAINS: term.value in v}[term.op]
    return r != term.negate


def expected_rows(table_rows, status, first, count, mask, terms):
    """the lines of [first, first + count) whose status is in mask and on which AND over the groups of
    (OR over the group's terms) holds; table_rows: {(path, kind): the column's decoded value per line}"""
    out = []
    for i in range(first, first + count):
        if not (mask >> int(status[i])) & 1:
            continue
        groups = {}
        for t in terms:
            groups.setdefault(t.group, []).append(term_holds(t, table_rows[(t.path, t.kind)][i]))
        if all(any(g) for g in groups.values()):
            out.append(i)
    return np.asarray(out, dtype=np.int64)


def decoded(table, columns):
    """{(path, kind): [None | int | bytes per line]} of BatchResult.table_from(res, columns, decode=False)"""
    out = {}
    for path, typ in columns:
        v, ok = table[path]
        if typ is str:
            off, chars = v
            raw = np.asarray(chars).tobytes()
            out[(path, str)] = [raw[off[j]:off[j + 1]] if ok[j] else None for j in range(len(ok))]
        else:
            out[(path, int)] = [int(v[j]) if ok[j] else None for j in range(len(ok))]
    return out
