"""Rate of the device map column (lp_result_table_map on a device view) beside
the 8-column typed table and a named query-parameter column, DESIGN.md §6.3.

    python tools/map_column_rate.py [--lines N] [--skew TILES] [--host-lines M] [--pkg DIR]

One process, one build: N config-2 lines in one batch (bench.py's generator
and seed), a handle with every path of 'combined'; three calls of bench.py's
device_table (the 8 TABLE_COLS), then -- when the package has the map column
-- four timed calls of table_map_device for STRING:request.firstline.uri.query.*
into buffers sized by a first call, and three of the named column
...query.q.  Phases are HIP events on the handle's stream (table_timing /
table_map_timing).  --skew TILES adds the skewed batch: the last batch of
tests/uri_wave_corpus.piece_cases() tiled TILES times; --host-lines M the host
path (table_map_from, 16 threads) on M lines.  --pkg DIR imports logparser_amd
from DIR (another checkout's package with its own built library: the parent
commit, to alternate the two builds).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = "STRING:request.firstline.uri.query.*"


def map_runs(r, path, calls):
    a = r.table_map_device([path], decode=False)[path]
    ne, nk, nv = a["key_off"].numel() - 1, a["key_chars"].numel(), a["val_chars"].numel()
    del a
    bufs = r.table_map_buffers([path], r.n_lines, ne, nk, nv)
    for t in bufs[0].values():
        t.zero_()
    import torch
    runs = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.table_map_device([path], buffers=bufs, decode=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ph = r.table_map_timing()
        ks = sum(ph.values()) / 1e3
        runs.append({"wall_s": round(dt, 4), "phase_ms": {k: round(v, 3) for k, v in ph.items()},
                     "rows_per_s_kernels": round(r.n_lines / ks, 1), "entries_per_s_kernels": round(ne / ks, 1),
                     "rows_per_s_wall": round(r.n_lines / dt, 1)})
    return {"entries": ne, "key_bytes": nk, "val_bytes": nv, "runs": runs}


def named_runs(r, path, calls):
    cols = [(path, str)]
    t = r.table_device(cols)
    tb = r.table_buffers(cols, chars_cap={k: int(v[0][1].numel()) + 16 for k, v in t.items()})
    out = []
    for _ in range(calls):
        r.table_device(cols, buffers=tb)
        ph = r.table_timing()
        out.append({"phase_ms": {k: round(v, 3) for k, v in ph.items()},
                    "rows_per_s_kernels": round(r.n_lines / (sum(ph.values()) / 1e3), 1)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--skew", type=int, default=0)
    ap.add_argument("--host-lines", type=int, default=0)
    ap.add_argument("--pkg", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    import logparser_amd as lpa
    import bench
    torch.cuda.set_device(0)
    has_map = hasattr(lpa.BatchResult, "table_map_device")
    p = lpa.HttpdLoglineParser("combined", lpa.get_possible_paths("combined"))
    res = {"lines": args.lines, "package": os.path.dirname(os.path.abspath(lpa.__file__))}
    buf, nbytes, _ = bench.generate_to_device(lpa, torch, 2, 0, args.lines, torch.device("cuda", 0))
    for _ in range(2):
        st = p.run(buf.data_ptr(), nbytes)
    res["parse"] = {k: st[k] for k in ("lines", "ok", "bad", "fallback", "ms_total")}
    res["table"] = []
    for _ in range(3):
        d = bench.device_table(lpa, torch, p, args.lines)
        res["table"].append({k: d[k] for k in ("table_rows_per_s_device", "table_rows_per_s_kernels", "table_phase_ms")})
    if has_map:
        r = lpa.BatchResult(p)
        res["map"] = map_runs(r, REQ, 4)
        res["named_column"] = named_runs(r, "STRING:request.firstline.uri.query.q", 3)
    del buf
    if has_map and args.skew:
        import uri_wave_corpus as uwc
        case = uwc.piece_cases()[-1]
        data = torch.frombuffer(bytearray(case.data), dtype=torch.uint8).repeat(args.skew).cuda()
        for _ in range(2):
            st = p.run(data.data_ptr(), data.numel())
        r = lpa.BatchResult(p)
        res["skew"] = {"lines": st["lines"], "ok": st["ok"], "bytes": data.numel(), "tile_lines": len(case.lines),
                       "tile_wave_pieces": case.wave_pieces(), "map": map_runs(r, REQ, 4),
                       "named_column": named_runs(r, "STRING:request.firstline.uri.query.k7", 3)}
        del data
    if has_map and args.host_lines:
        r = p.parse_batch(lpa.synth_combined(bench.SEEDS[2], 0, args.host_lines))
        hbuf, hres = r.copy_to_host()  # (hres points into hbuf)
        res["host"] = []
        for _ in range(3):
            t0 = time.perf_counter()
            h = r.table_map_from(hres, [REQ], threads=16, decode=False)  # two calls: the sizes, then the arrays
            dt = time.perf_counter() - t0
            res["host"].append({"rows_per_s": round(r.n_lines / dt, 1), "entries": int(h[REQ]["key_off"].size - 1),
                                "seconds": round(dt, 4)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
