"""Corpora and helpers of the dictionary-column tests (lp_result_table_dict),
shared by test_table_dict.py (CPU) and test_table_dict_gpu.py.

The truth of a dictionary column is the project's own plain STRING column of
the same rows: expected_dict factorises it by first occurrence in pure numpy."""
import numpy as np

FMT = "combined"
UA = "HTTP.USERAGENT:request.user-agent"
PATH = "HTTP.PATH:request.firstline.uri.path"
QUERY = "HTTP.QUERYSTRING:request.firstline.uri.query"  # the raw query string: a leading '&' (SW_AMP)
STATUS = "STRING:request.status.last"
BYTES = "BYTES:response.body.bytes"  # ConvertCLFIntoNumber: a long rendered as text, "-" -> 0 (SW_LONG)
DATE = "TIME.DATE:request.receive.time.date"  # formatted (SW_SLOW)
MONTHNAME = "TIME.MONTHNAME:request.receive.time.monthname"
METHOD = "HTTP.METHOD:request.firstline.method"
REFERER = "HTTP.URI:request.referer"
PARAM_A = "STRING:request.firstline.uri.query.a"
PARAM_E = "STRING:request.firstline.uri.query.e"  # "" in every line of line()
REQ = "STRING:request.firstline.uri.query.*"
COMMON_FIELDS = [STATUS, METHOD, PATH, BYTES]  # delivered by 'common' too

_LINE = b'10.0.%d.%d - - [%02d/%s/2026:13:55:36 +0200] "%s %s?e=&a=%s HTTP/1.1" %d %s "%s" "%s"'
_MONTHS = (b"Jan", b"Feb", b"Mar", b"Oct", b"Dec")


def line(k, ua=b"Mozilla/5.0 (X11)", path=None, a=None, method=b"GET", status=None, size=None, ref=b"-"):
    """an OK 'combined' line; by default a handful of distinct values per column"""
    path = b"/p%d" % (k % 7) if path is None else path
    a = b"%d" % (k % 5) if a is None else a
    status = (200, 404, 301)[k % 3] if status is None else status
    size = (b"-" if k % 4 == 0 else b"%d" % (k % 6 * 1000)) if size is None else size
    return _LINE % (k // 256 % 256, k % 256, 1 + k % 28, _MONTHS[k % 5], method, path, a, status, size, ref, ua)


def common_line(k):
    """the same request as an OK 'common' line (no referer, no user agent)"""
    return line(k).rsplit(b' "', 2)[0]


def join_lf(lines):
    return b"".join(l + b"\n" for l in lines)


def expected_dict(off, chars, valid):
    """First-occurrence factorisation of a plain Arrow STRING column (offsets
    [n + 1], chars, valid [n]): (index int32 [n], dict_off int64 [d + 1],
    dict_chars uint8).  A row that is not valid has index 0 and contributes no
    entry; "" is a value; entry j is the value whose first valid row comes j-th."""
    off = np.asarray(off, dtype=np.int64)
    b = np.asarray(chars, dtype=np.uint8).tobytes()
    valid = np.asarray(valid)
    n = len(off) - 1
    index = np.zeros(n, dtype=np.int32)
    seen, entries = {}, []
    for k in range(n):
        if not valid[k]:
            continue
        v = b[off[k]:off[k + 1]]
        j = seen.get(v)
        if j is None:
            j = seen[v] = len(entries)
            entries.append(v)
        index[k] = j
    dict_off = np.zeros(len(entries) + 1, dtype=np.int64)
    if entries:
        np.cumsum([len(e) for e in entries], out=dict_off[1:])
    return index, dict_off, np.frombuffer(b"".join(entries), dtype=np.uint8)
