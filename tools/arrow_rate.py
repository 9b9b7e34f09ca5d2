"""The Arrow export (lp_result_arrow on a device view) beside the existing table
calls for the same columns, DESIGN.md "Arrow export".

    python tools/arrow_rate.py [--lines N] [--runs K] [--pkg DIR] [--tables-only]

One process: N config-2 lines in one batch (bench.py's generator and seed), a
handle with every path of 'combined' and the request's query wildcard.  Two
column sets: bench.py's 8-column table, and the same plus one dictionary column
(the user agent) and one map column (the request's query wildcard).  Per set,
after one warm-up call, K timed calls each of

  tables       lp_result_table (/ _dict / _map) into buffers sized beforehand:
               wall time (the calls return synchronised) and their HIP-event phases;
  tables_2pass the same calls with the size protocol (a first call that reports
               the sizes, buffers from torch's caching allocator, a second call);
  arrow        lp_result_arrow on the device view, released after each call:
               wall time and lp_last_timing [16], the packaging kernels; from it
               the packaging's algorithmic bytes (1.125 B per row per nullable
               column, 12 B per map row) over that time.

--pkg DIR imports logparser_amd from another checkout (the parent commit's
build) and --tables-only skips what that build does not have.  Prints one JSON
line; what is left of `arrow` after `tables_2pass` and the packaging is
allocation (hipMalloc / hipFree of every buffer) and the wrapping.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQ = "STRING:request.firstline.uri.query.*"
UA = "HTTP.USERAGENT:request.user-agent"
HBM_GBS = 8000.0  # MI355X peak HBM bandwidth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pkg", default=ROOT)
    ap.add_argument("--tables-only", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import bench
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    import logparser_amd as lpa
    torch.cuda.set_device(0)
    fields = [f for f in lpa.get_possible_paths("combined") if not f.endswith("*")] + [REQ]
    p = lpa.HttpdLoglineParser("combined", fields)
    buf, nbytes, _ = bench.generate_to_device(lpa, torch, 2, 0, args.lines, torch.device("cuda", 0))
    for _ in range(2):
        st = p.run(buf.data_ptr(), nbytes)
    r = lpa.BatchResult(p)
    n = r.n_lines
    plain = list(bench.TABLE_COLS)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def tables(sets, sized):
        """the existing calls for the plain (+ dict + map) columns; sized: {} buffers made beforehand"""
        ms = {}
        t, _ = wall(lambda: r.table_device(plain, buffers=sized.get("plain")))
        ms["table"] = t
        ms["table_phases"] = {k: round(v, 3) for k, v in r.table_timing().items()}
        if sets == "all":
            t, _ = wall(lambda: r.table_dict_device([UA], buffers=sized.get("dict")))
            ms["dict"] = t
            t, _ = wall(lambda: r.table_map_device([REQ], buffers=sized.get("map"), decode=False))
            ms["map"] = t
        ms["total"] = round(sum(v for k, v in ms.items() if k in ("table", "dict", "map")), 3)
        return {k: round(v, 3) if isinstance(v, float) else v for k, v in ms.items()}

    out = {"lines": n, "input_bytes": nbytes, "pkg": os.path.abspath(args.pkg), "runs": args.runs,
           "parse": {k: st[k] for k in ("ok", "bad", "fallback", "ms_total")}, "sets": {}}
    for sets in ("plain8", "all"):
        res = {}
        # buffers of the exact sizes, made and touched beforehand
        t = r.table_device(plain)
        caps = {pth: int(v[0][1].numel()) + 16 for pth, v in t.items() if dict(plain)[pth] is str}
        del t
        sized = {"plain": r.table_buffers(plain, chars_cap=caps)}
        if sets == "all":
            d = r.table_dict_device([UA])[UA]
            sized["dict"] = r.table_dict_buffers([UA], dict_cap=int(d[1][0].numel()) - 1, dict_chars_cap=int(d[1][1].numel()))
            m = r.table_map_device([REQ], decode=False)[REQ]
            sized["map"] = r.table_map_buffers([REQ], entries_cap=int(m["key_off"].numel()) - 1,
                                               key_chars_cap=int(m["key_chars"].numel()), val_chars_cap=int(m["val_chars"].numel()))
            res["map_entries"] = int(m["key_off"].numel()) - 1
            del d, m
        tables(sets, sized)  # warm-up
        res["tables"] = [tables(sets, sized) for _ in range(args.runs)]
        del sized
        torch.cuda.empty_cache()
        tables(sets, {})
        res["tables_2pass"] = [tables(sets, {}) for _ in range(args.runs)]
        torch.cuda.empty_cache()
        if not args.tables_only:
            cols = plain + ([(UA, "dict"), (REQ, "map")] if sets == "all" else [])
            nullable = len(cols)
            pack_bytes = 1.125 * n * nullable + (12 * n if sets == "all" else 0)
            runs = []
            for k in range(args.runs + 1):
                t, e = wall(lambda: r.to_arrow_device(cols))
                pack = r.arrow_timing()
                tr, _ = wall(e.release)
                if k:  # (the first call is the warm-up)
                    runs.append({"call_ms": round(t, 3), "pack_ms": round(pack, 4), "release_ms": round(tr, 3),
                                 "pack_gbs": round(pack_bytes / pack / 1e6, 1) if pack > 0 else None,
                                 "pack_fraction_of_hbm": round(pack_bytes / pack / 1e6 / HBM_GBS, 4) if pack > 0 else None})
                del e
            res["arrow"] = runs
            res["pack_algorithmic_bytes"] = int(pack_bytes)
        out["sets"][sets] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
