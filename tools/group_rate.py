"""Grouped aggregates (lp_result_group): count and sum of BYTES per key beside
the calls a user needs for the same inputs without it -- lp_result_table_dict
of the key plus lp_result_table of the measure -- DESIGN.md §6.16.

    python tools/group_rate.py [--lines N] [--runs K]

One process, one build: N config-2 lines (bench.py's generator and seed)
resident in HBM, a handle with every path of 'combined' and the request's query
wildcard.  Per key (method, status, user agent, the query parameter the
generator uses most, path), K calls each, timed with HIP events
(lp_last_timing):
  group      group_device([(key, str)], [COUNT_ROWS, SUM BYTES]) with room for
             the groups allotted: group_timing's insert / index / aggregate, the
             regime that ran (groups x 3 words against the default LDS budget)
             and the bytes the call writes to the caller (group_of, rep, the
             two aggregates)
  yardstick  table_dict_device of the key into sized buffers (its four phases)
             plus table_device of BYTES as a LONG column (its values phase),
             and the bytes those write
and, for every key, the direct regime forced (OPT_GROUP_LDS_WORDS -1) with the
default peel rounds and without the peel (OPT_GROUP_PEEL -1): the measurement
behind the defaults.  Prints one JSON line.
"""
import argparse
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [("method", "HTTP.METHOD:request.firstline.method"), ("status", "STRING:request.status.last"),
        ("user_agent", "HTTP.USERAGENT:request.user-agent"), ("path", "HTTP.PATH:request.firstline.uri.path")]
REQ = "STRING:request.firstline.uri.query.*"
BYTES = "BYTES:response.body.bytes"


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
    keys = list(KEYS)
    if names:
        keys.insert(3, ("query_param", "STRING:request.firstline.uri.query." + names.most_common(1)[0][0].decode()))
    aggs = [lpa.Agg(lpa.AGG_COUNT_ROWS), lpa.Agg(lpa.AGG_SUM, BYTES)]
    words = lpa.group_acc_words(aggs)
    out = {"lines": n, "input_bytes": nbytes, "runs": args.runs,
           "parse": {k: st[k] for k in ("ok", "bad", "fallback", "ms_total")},
           "acc_words_per_group": words, "lds_budget_words": lpa.GROUP_LDS_WORDS,
           "scratch_formula_bytes": 41 * n, "keys": {}}
    L, h = lpa.lib(), p._h

    def group_runs(key, lds, peel, cap):
        L.lp_set_option(h, lpa.OPT_GROUP_LDS_WORDS, lds)
        L.lp_set_option(h, lpa.OPT_GROUP_PEEL, peel)
        runs = []
        try:
            for _ in range(args.runs):
                g = r.group_device([(key, str)], aggs, groups_cap=cap)
                t = r.group_timing()
                runs.append({k: round(v, 3) for k, v in t.items()} | {"total": round(sum(t.values()), 3)})
                del g
        finally:
            L.lp_set_option(h, lpa.OPT_GROUP_LDS_WORDS, 0)
            L.lp_set_option(h, lpa.OPT_GROUP_PEEL, 0)
        return runs

    for name, path in keys:
        g = r.group_device([(path, str)], aggs)  # sizes
        n_groups = g["n_groups"]
        top = int(g["aggs"][0][0].max().item())
        del g
        need = n_groups * words
        e = {"path": path, "n_groups": n_groups, "largest_group_rows": top, "acc_words_needed": need,
             "regime": "privatised" if need <= lpa.GROUP_LDS_WORDS else "direct",
             "group_ms": group_runs(path, 0, 0, n_groups),
             "group_output_bytes": 4 * n + 8 * n_groups + 2 * 9 * n_groups,
             "direct_peel_ms": group_runs(path, -1, 0, n_groups),
             "direct_no_peel_ms": group_runs(path, -1, -1, n_groups)}
        # the yardstick: the key's dictionary column and the measure's LONG column
        d = r.table_dict_device([path])
        idx, (doff, dchars), valid = d[path]
        dict_len, dict_bytes = int(doff.numel()) - 1, int(dchars.numel())
        del d, idx, doff, dchars, valid
        bufs = r.table_dict_buffers([path], dict_cap=dict_len, dict_chars_cap=dict_bytes)
        mb = r.table_buffers([(BYTES, int)])
        yruns = []
        for _ in range(args.runs):
            r.table_dict_device([path], buffers=bufs)
            td = r.table_dict_timing()
            r.table_device([(BYTES, int)], buffers=mb)
            tt = r.table_timing()
            yruns.append({"dict": round(sum(td.values()), 3), "measure": round(sum(tt.values()), 3),
                          "total": round(sum(td.values()) + sum(tt.values()), 3)})
        del bufs, mb
        torch.cuda.empty_cache()
        e["yardstick_ms"] = yruns
        e["yardstick_output_bytes"] = (n + 4 * n + 8 * (dict_len + 1) + dict_bytes) + (n + 8 * n)
        out["keys"][name] = e
    print(json.dumps(out))


if __name__ == "__main__":
    main()
