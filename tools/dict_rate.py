"""Dictionary-encoded STRING columns (lp_result_table_dict) beside the plain
STRING column of the same path on the same build, DESIGN.md "Dictionary
columns".

    python tools/dict_rate.py [--lines N] [--runs K]

One process, one build: N config-2 lines in one batch (bench.py's generator
and seed), a handle with every path of 'combined' and the request's query
wildcard.  Per column (method, status, referer, user agent, path, the query
parameter the generator uses most): K calls of table_dict_device into sized
buffers (table_dict_timing's phases, HIP events) and K calls of table_device
for the plain column (table_timing's phases); the output bytes both ways,
dict_len and the scratch formula of a dictionary column (44 bytes per row; the
engine's allocation adds the scans' temporaries, 64 KiB and alignment,
csrc/kernels.h DictLayout).  Prints one JSON line.
"""
import argparse
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = [("method", "HTTP.METHOD:request.firstline.method"), ("status", "STRING:request.status.last"),
           ("referer", "HTTP.URI:request.referer"), ("user_agent", "HTTP.USERAGENT:request.user-agent"),
           ("path", "HTTP.PATH:request.firstline.uri.path")]
REQ = "STRING:request.firstline.uri.query.*"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import logparser_amd as lpa
    import bench
    torch.cuda.set_device(0)
    fields = [f for f in lpa.get_possible_paths("combined") if not f.endswith("*")] + [REQ]
    p = lpa.HttpdLoglineParser("combined", fields)
    buf, nbytes, _ = bench.generate_to_device(lpa, torch, 2, 0, args.lines, torch.device("cuda", 0))
    for _ in range(2):
        st = p.run(buf.data_ptr(), nbytes)
    r = lpa.BatchResult(p)
    n = r.n_lines
    head = bytes(buf[:1 << 20].cpu().numpy().tobytes())
    names = collections.Counter(x for u in re.findall(rb'"[A-Z]+ (\S+) HTTP', head) for x in re.findall(rb"[?&]([a-z0-9_]+)=", u))
    cols = list(COLUMNS)
    if names:
        cols.append(("query_param", "STRING:request.firstline.uri.query." + names.most_common(1)[0][0].decode()))
    out = {"lines": n, "input_bytes": nbytes, "parse": {k: st[k] for k in ("ok", "bad", "fallback", "ms_total")},
           "scratch_formula_bytes_per_dict_column": 44 * n,
           "scratch_note": "the formula's 44 bytes per row (csrc/kernels.h DictLayout), not read from the engine: the "
                           "allocation adds the scans' temporaries, 64 KiB and 256-byte alignment of each array",
           "columns": {}}
    for name, path in cols:
        d = r.table_dict_device([path])  # sizes
        idx, (doff, dchars), valid = d[path]
        dict_len, dict_bytes = int(doff.numel()) - 1, int(dchars.numel())
        del d, idx, doff, dchars, valid
        bufs = r.table_dict_buffers([path], dict_cap=dict_len, dict_chars_cap=dict_bytes)
        druns = []
        for _ in range(args.runs):
            r.table_dict_device([path], buffers=bufs)
            t = r.table_dict_timing()
            druns.append({k: round(v, 3) for k, v in t.items()} | {"total": round(sum(t.values()), 3)})
        del bufs
        t = r.table_device([(path, str)])
        plain_bytes = int(t[path][0][1].numel())
        del t
        pb = r.table_buffers([(path, str)], chars_cap=plain_bytes + 16)
        pruns = []
        for _ in range(args.runs):
            r.table_device([(path, str)], buffers=pb)
            t = r.table_timing()
            pruns.append({k: round(v, 3) for k, v in t.items()} | {"total": round(sum(t.values()), 3)})
        del pb
        torch.cuda.empty_cache()
        out["columns"][name] = {
            "path": path, "dict_len": dict_len, "dict_ms": druns, "plain_ms": pruns,
            "dict_output_bytes": n + 4 * n + 8 * (dict_len + 1) + dict_bytes,
            "plain_output_bytes": n + 8 * (n + 1) + plain_bytes,
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
