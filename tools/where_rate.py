"""Predicate row selection (lp_result_select_where): the predicate pass and its
compaction beside the route the parent commit offers -- the one-column device
table of the predicate's column -- and the end-to-end "8 columns of the
selected lines" against the whole-batch table, DESIGN.md §6.15.

    python tools/where_rate.py [--lines N] [--reps K]

One process, one build: N config-2 lines (bench.py's generator and seed)
resident in HBM, a handle with every path of 'combined'.  Per case, medians
over K calls after two warm-up calls:
  where    select_where_device: lp_last_timing [18] (k_where_eval), [19] (the
           compaction: count pass, block scan, the host's read of the total,
           write pass), and the wall time of the sized call pair
  column   table_device of the one column into sized buffers: table_timing's
           values / scans / chars (a LONG column has only values)
The cases: (a) the status class as text, STRING:request.status.last PREFIX "5"
(the path's casts are STRING only), and a LONG range, BYTES:response.body.bytes
BETWEEN 500 AND 599; (b) HTTP.PATH PREFIX; (c) the user agent CONTAINS; (d)
"@line" CONTAINS.  Then bench.py's 8 TABLE_COLS over the rows of (a) against
the whole-batch table.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def med(xs):
    return round(statistics.median(xs), 4)


def sized_buffers(r, cols, rows=None):
    kw = {"rows": rows} if rows is not None else {}
    t = r.table_device(cols, **kw)
    caps = {p: int(v[0][1].numel()) + 16 for p, v in t.items() if dict(cols)[p] is str}
    del t
    return r.table_buffers(cols, chars_cap=caps, **kw)


def table_runs(torch, r, cols, reps, rows=None):
    kw = {"rows": rows} if rows is not None else {}
    bufs = sized_buffers(r, cols, rows)
    ph, wall = [], []
    for k in range(reps + 2):
        _t, dt = timed(torch, lambda: r.table_device(cols, buffers=bufs, **kw))
        if k >= 2:
            ph.append(r.table_timing())
            wall.append(dt * 1e3)
    del bufs
    out = {k: med([p[k] for p in ph]) for k in ("values", "scans", "chars")}
    out["sum_ms"] = round(sum(out.values()), 4)
    out["wall_ms"] = med(wall)
    return out


def where_runs(torch, r, terms, reps):
    pred, comp, wall = [], [], []
    rows = None
    for k in range(reps + 2):
        rows, dt = timed(torch, lambda: r.select_where_device(terms))
        if k >= 2:
            a, b = r.select_where_timing()
            pred.append(a)
            comp.append(b)
            wall.append(dt * 1e3)
    return rows, {"selected": int(rows.numel()), "predicate_ms": med(pred), "compaction_ms": med(comp),
                  "sum_ms": round(med(pred) + med(comp), 4), "wall_ms_two_calls": med(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import logparser_amd as lpa
    import bench
    torch.cuda.set_device(0)
    W = lpa.Where
    p = lpa.HttpdLoglineParser("combined", lpa.get_possible_paths("combined"))
    buf, nbytes, _ = bench.generate_to_device(lpa, torch, 2, 0, args.lines, torch.device("cuda", 0))
    for _ in range(2):
        st = p.run(buf.data_ptr(), nbytes)
    r = lpa.BatchResult(p)
    res = {"lines": r.n_lines, "input_bytes": nbytes, "reps": args.reps,
           "parse": {k: st[k] for k in ("lines", "ok", "bad", "fallback", "ms_total")}}
    status, nbytes_col = "STRING:request.status.last", "BYTES:response.body.bytes"
    path, ua = "HTTP.PATH:request.firstline.uri.path", "HTTP.USERAGENT:request.user-agent"
    # operands that occur: the first line's path prefix and a word of its user agent
    first = r.table_device([(path, str), (ua, str)], first=0, count=1)
    pv = bytes(first[path][0][1].cpu().numpy().tobytes())
    uv = bytes(first[ua][0][1].cpu().numpy().tobytes())
    cases = [("a_status_prefix_5", [W(status, lpa.WHERE_PREFIX, "5")], (status, str)),
             ("a_bytes_between_500_599", [W(nbytes_col, lpa.WHERE_BETWEEN, 500, 599)], (nbytes_col, int)),
             ("b_path_prefix", [W(path, lpa.WHERE_PREFIX, pv[:max(1, len(pv) // 2)])], (path, str)),
             ("c_useragent_contains", [W(ua, lpa.WHERE_CONTAINS, uv[len(uv) // 2:len(uv) // 2 + 6])], (ua, str)),
             ("d_line_contains", [W("@line", lpa.WHERE_CONTAINS, uv[len(uv) // 2:len(uv) // 2 + 6])], ("@line", str))]
    res["cases"] = {}
    rows_a = None
    for name, terms, col in cases:
        rows, w = where_runs(torch, r, terms, args.reps)
        if rows_a is None:
            rows_a = rows
        res["cases"][name] = {"terms": [repr(t) for t in terms], "where": w, "column": table_runs(torch, r, [col], args.reps)}
        del rows
    # the 8 columns of the (a) lines against the whole-batch table
    cols = [c for c in bench.TABLE_COLS if c[0] in p.fields]
    _rows, w = where_runs(torch, r, cases[0][1], args.reps)
    res["eight_columns"] = {"columns": [c for c, _ in cols], "rows": int(rows_a.numel()), "where": w,
                            "table_rows": table_runs(torch, r, cols, args.reps, rows=rows_a),
                            "table_whole_batch": table_runs(torch, r, cols, max(2, args.reps // 2))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
