"""Row selection (lp_result_select, lp_result_table_rows, the pseudo-columns):
the contiguous path's rate beside the parent commit's, and the feature's own
rates, DESIGN.md §6.5.

    python tools/row_select_rate.py [--lines N] [--pkg DIR] [--feature]

One process, one build.  Always: N config-2 lines in one batch (bench.py's
generator and seed), a handle with every path of 'combined'; three calls of
bench.py's device_table (the 8 TABLE_COLS: table_timing's values / scans /
chars) and four of table_map_device for STRING:request.firstline.uri.query.*
into sized buffers (table_map_timing's count / entries / fill) -- the window
calls, which --pkg DIR measures on another checkout's package with its own
built library (the parent commit, to alternate the two builds).

--feature (a package with select_device): N config-3 lines (5 % malformed):
  select      select_device(SEL_OK), HIP events and wall; the select pass as a
              fraction of the HBM roofline for its algorithmic bytes (N status
              bytes read twice, 8 bytes per selected row written)
  dense       the 8-column table over those rows, against the whole-batch
              table followed by a host-side compaction of the copied columns
  fallback    select_device(SEL_BAD | SEL_FALLBACK) plus an "@line" /
              "@lineno" table of those rows, against lp_line_status plus a copy
              of the whole input
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = "STRING:request.firstline.uri.query.*"


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def sized_buffers(r, cols, rows=None):
    t = r.table_device(cols, rows=rows) if rows is not None else r.table_device(cols)
    caps = {p: int(v[0][1].numel()) + 16 for p, v in t.items() if dict(cols)[p] is str}
    del t
    bufs = r.table_buffers(cols, chars_cap=caps, rows=rows) if rows is not None else r.table_buffers(cols, chars_cap=caps)
    for b in bufs:
        for x in b:
            if x is not None:
                x.zero_()
    return bufs


def feature(lpa, torch, bench, lines):
    import numpy as np
    fmt = lpa.SYNTH_FORMATS[lpa.SYNTH_STRFTIME]
    p = lpa.HttpdLoglineParser(fmt, lpa.get_possible_paths(fmt))
    buf, nbytes, _ = bench.generate_to_device(lpa, torch, 3, 0, lines, torch.device("cuda", 0))
    for _ in range(2):
        st = p.run(buf.data_ptr(), nbytes)
    r = lpa.BatchResult(p)
    n = r.n_lines
    out = {"lines": n, "ok": st["ok"], "bad": st["bad"], "fallback": st["fallback"], "input_bytes": nbytes}
    # select
    runs = []
    for _ in range(5):
        rows, dt = timed(torch, lambda: r.select_device(lpa.SEL_OK))
        ms = r.select_timing()
        b = 2 * n + 8 * int(rows.numel())
        runs.append({"wall_s": round(dt, 5), "kernels_ms": round(ms, 3), "algorithmic_bytes": b,
                     "gbs": round(b / (ms / 1e3) / 1e9, 1), "roofline_frac": round(b / (ms / 1e3) / 1e9 / bench.HBM_PEAK_GBS, 4)})
    out["select_ok"] = {"selected": int(rows.numel()), "runs": runs,
                        "note": "wall: two lp_result_select calls (the count, then the rows); kernels_ms: the second "
                                "call's count pass, scan, read of the count and write pass (lp_last_timing [11])"}
    # the dense table over the OK rows, against the whole-batch table and a host-side compaction
    cols = [c for c in bench.TABLE_COLS if c[0] in p.fields]
    bufs = sized_buffers(r, cols, rows)
    dense = []
    for _ in range(3):
        _t, dt = timed(torch, lambda: r.table_device(cols, buffers=bufs, rows=rows))
        dense.append({"wall_s": round(dt, 4), "phase_ms": {k: round(v, 3) for k, v in r.table_timing().items()}})
    del bufs
    bufs = sized_buffers(r, cols)
    whole = []
    for k in range(2):
        t, dt = timed(torch, lambda: r.table_device(cols, buffers=bufs))
        ph = {k2: round(v, 3) for k2, v in r.table_timing().items()}
        t0 = time.perf_counter()
        keep = torch.from_numpy(r.status == lpa.LINE_OK)
        idx = np.nonzero(keep.numpy())[0]
        host = {}
        for path, typ in cols:
            v, ok = t[path]
            if typ is str:
                off, chars = v[0].cpu().numpy(), v[1].cpu().numpy()
                # (a row that is not OK holds no bytes: the bytes are dense already, the offsets are not)
                host[path] = (np.append(off[idx], off[-1]), chars, ok.cpu().numpy()[idx])
            else:
                host[path] = (v.cpu().numpy()[keep.numpy()], ok.cpu().numpy()[keep.numpy()])
        tc = time.perf_counter() - t0
        whole.append({"table_wall_s": round(dt, 4), "phase_ms": ph, "copy_and_compact_s": round(tc, 3)})
        del host, t
    del bufs
    out["dense_table"] = {"columns": [c for c, _ in cols], "rows": int(rows.numel()), "device_rows": dense,
                          "whole_then_host_compaction": whole}
    # the lines the host must redo: their text and numbers, against the statuses plus the whole input
    pcols = [("@line", str), ("@lineno", int)]
    redo = []
    for _ in range(3):
        def dev():
            rr = r.select_device(lpa.SEL_BAD | lpa.SEL_FALLBACK)
            return rr, r.table_device(pcols, rows=rr)
        (rr, t), dt = timed(torch, dev)
        _h, dth = timed(torch, lambda: (t["@line"][0][0].cpu(), t["@line"][0][1].cpu(), t["@lineno"][0].cpu()))
        redo.append({"select_and_table_s": round(dt, 4), "copy_to_host_s": round(dth, 4), "rows": int(rr.numel()),
                     "line_bytes": int(t["@line"][0][1].numel())})
        del t
    base = []
    stat = np.zeros(n, dtype=np.uint8)
    for _ in range(2):
        t0 = time.perf_counter()
        lpa.lib().lp_line_status(p._h, 0, n, stat.ctypes.data)
        t1 = time.perf_counter()
        hostbuf = buf[:nbytes].cpu()
        t2 = time.perf_counter()
        base.append({"line_status_s": round(t1 - t0, 4), "input_copy_s": round(t2 - t1, 3)})
        del hostbuf
    out["redo_lines"] = {"device": redo, "status_plus_input_copy": base}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--pkg", default=ROOT)
    ap.add_argument("--feature", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    import logparser_amd as lpa
    import bench
    import map_column_rate as mcr
    torch.cuda.set_device(0)
    res = {"lines": args.lines, "package": os.path.dirname(os.path.abspath(lpa.__file__))}
    p = lpa.HttpdLoglineParser("combined", lpa.get_possible_paths("combined"))
    buf, nbytes, _ = bench.generate_to_device(lpa, torch, 2, 0, args.lines, torch.device("cuda", 0))
    for _ in range(2):
        st = p.run(buf.data_ptr(), nbytes)
    res["parse"] = {k: st[k] for k in ("lines", "ok", "bad", "fallback", "ms_total")}
    res["table"] = []
    for _ in range(3):
        d = bench.device_table(lpa, torch, p, args.lines)
        res["table"].append({k: d[k] for k in ("table_rows_per_s_kernels", "table_phase_ms")})
    res["map"] = mcr.map_runs(lpa.BatchResult(p), REQ, 4)
    del buf, p
    if args.feature:
        res["feature"] = feature(lpa, torch, bench, args.lines)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
