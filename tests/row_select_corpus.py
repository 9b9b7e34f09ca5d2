"""Corpora and helpers of the row-selection tests (lp_result_select, the *_rows
tables, the pseudo-columns), shared by test_row_select.py (CPU: the helpers and
the planted statuses) and test_row_select_gpu.py.

Batches are built from explicit lines with all three statuses planted at known
positions: OK lines are 'combined' lines, BAD lines are b"garbage" (or empty),
FALLBACK lines are 'combined' lines with a 0x7F byte in the user agent
(the FALLBACK subset) -- one of them longer than 8191
bytes, one holding invalid UTF-8."""
import numpy as np

import corpora

OK, BAD, FALLBACK = 0, 1, 2
FMT = "combined"

_LINE = b'10.0.%d.%d - u%d [10/Oct/2026:13:55:36 +0200] "GET /p%d?a=%d&k7=v%d&a=z HTTP/1.1" 200 %d "%s" "%s"'


def ok_line(k, ua=b"Mozilla/5.0 (X11)"):
    ref = b"http://h.example.com/r?x=%d" % k if k % 3 else b"-"
    return _LINE % (k // 256 % 256, k % 256, k, k, k, k, 100 + k % 900, ref, ua)


def bad_line(k):
    return b"garbage"


def fallback_line(k, extra=b""):
    return ok_line(k, ua=b"ua\x7f" + extra)


def planted():
    """[(line, status)]: the three statuses interleaved, runs of each, the
    special lines; 200 lines (more than three waves of 64 rows)"""
    out = []
    for k in range(200):
        if k == 5:
            out.append((fallback_line(k, b"x" * 9000), FALLBACK))      # longer than 8191 bytes
        elif k == 9:
            out.append((fallback_line(k, b"\xff\xfe\xc3("), FALLBACK))  # invalid UTF-8
        elif k == 11:
            out.append((b"", BAD))                                      # an empty line
        elif k % 7 == 3 or 64 <= k < 70:
            out.append((bad_line(k), BAD))
        elif k % 11 == 6 or 128 <= k < 131:
            out.append((fallback_line(k), FALLBACK))
        else:
            out.append((ok_line(k), OK))
    return out


def pattern_lines(n, pattern):
    """n lines: 'ok' all OK, 'none' no OK line (BAD / FALLBACK alternating),
    'third' every third BAD, 'mixed' all three statuses (runs of 1 to 3 OK lines between the others)"""
    if pattern == "ok":
        return [(ok_line(k), OK) for k in range(n)]
    if pattern == "none":
        return [(bad_line(k), BAD) if k % 2 else (fallback_line(k), FALLBACK) for k in range(n)]
    if pattern == "mixed":
        return [(bad_line(k), BAD) if k % 5 == 2 else (fallback_line(k), FALLBACK) if k % 7 == 4 else (ok_line(k), OK)
                for k in range(n)]
    assert pattern == "third"
    return [(bad_line(k), BAD) if k % 3 == 2 else (ok_line(k), OK) for k in range(n)]


def join_lf(lines):
    return b"".join(l + b"\n" for l in lines)


def variants(lines, seed=3):
    """{name: buffer} of the same lines: '\\n' after each; "\\r\\n" / lone '\\r' /
    '\\n' mixed with no final terminator (corpora.crlf_join); '\\n' with no final
    terminator.  corpora.split_hadoop gives the lines of each back -- except an
    empty LAST line without terminator, which no reader sees: callers end on
    a non-empty line."""
    assert lines[-1] != b""
    out = {"lf": join_lf(lines), "crlf": corpora.crlf_join(lines, seed), "lonecr": corpora.crlf_join(lines, seed + 1, 0.6),
           "unterminated": join_lf(lines)[:-1]}
    for name, data in out.items():
        assert corpora.split_hadoop(data) == list(lines), name
    return out


def expected_rows(status, first, count, mask):
    """the lines of [first, first + count) whose status is in mask, ascending (pure numpy)"""
    status = np.asarray(status, dtype=np.uint8)
    window = status[first:first + count]
    return (first + np.nonzero((mask >> window.astype(np.int64)) & 1)[0]).astype(np.int64)


def gather_arrow(offsets, chars, valid, rows):
    """rows of a whole-batch Arrow STRING column (offsets [n + 1], chars, valid
    [n]) as the column of those rows: (offsets [len(rows) + 1], chars, valid)"""
    offsets, chars, valid = np.asarray(offsets), np.asarray(chars), np.asarray(valid)
    rows = np.asarray(rows, dtype=np.int64)
    lens = offsets[rows + 1] - offsets[rows] if len(rows) else np.zeros(0, np.int64)
    out_off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=out_off[1:])
    parts = [chars[offsets[r]:offsets[r + 1]] for r in rows]
    out_chars = np.concatenate(parts) if parts else np.zeros(0, dtype=chars.dtype)
    return out_off, out_chars.astype(np.uint8), valid[rows].astype(np.uint8)


def gather_map(arrays, rows):
    """rows of a whole-batch Arrow map column ({name: array}, logparser_amd.MAP_ARRAYS)
    as the column of those rows, every offset rebased to zero"""
    a = {n: np.asarray(v) for n, v in arrays.items()}
    rows = np.asarray(rows, dtype=np.int64)
    eo = a["entry_off"]
    ents = np.concatenate([np.arange(eo[r], eo[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = {"valid": a["valid"][rows].astype(np.uint8), "entry_off": np.zeros(len(rows) + 1, dtype=np.int64)}
    if len(rows):
        np.cumsum(eo[rows + 1] - eo[rows], out=out["entry_off"][1:])
    for off, ch in (("key_off", "key_chars"), ("val_off", "val_chars")):
        o = a[off]
        out[off] = np.zeros(len(ents) + 1, dtype=np.int64)
        if len(ents):
            np.cumsum(o[ents + 1] - o[ents], out=out[off][1:])
        parts = [a[ch][o[e]:o[e + 1]] for e in ents]
        out[ch] = (np.concatenate(parts) if parts else np.zeros(0, np.uint8)).astype(np.uint8)
    return out
