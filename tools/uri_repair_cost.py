"""Cost of the URI repair path: a config-2 corpus in which a share of the
request URIs end in a bad '%' escape (the last byte of the URI overwritten
in HBM, so the corpus keeps its size), parsed like bench.py's timed steps.

    python tools/uri_repair_cost.py [--lines N] [--percent P] [--steps K] [--warmup W]

Prints one JSON line: the planted lines, the status counts, the lines whose
URI stages were redone (diag uri_repair_lines; 0 with a library without the
repair: those lines are FALLBACK there) and the step / URI kernel times.
LOGPARSER_AMD_LIB selects the engine library, as for bench.py.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plant(torch, buf, off, nbytes, every, piece=1 << 28):
    """overwrites the last byte of every `every`-th request URI (the byte
    before ' HTTP/') with '%'; returns how many"""
    pat = torch.tensor(list(b" HTTP/"), dtype=torch.uint8, device=buf.device)
    seen = planted = 0
    for s in range(off, off + nbytes, piece):
        e = min(s + piece + len(pat), off + nbytes)
        x = buf[s:e]
        hit = x[:len(x) - 5] == pat[0]
        for k in range(1, 6):
            hit &= x[k:len(x) - 5 + k] == pat[k]
        pos = torch.nonzero(hit[:piece]).flatten() + s
        pos = pos[pos >= off + 4]
        # the URI has at least three bytes (no blank among its last three)
        pos = pos[(buf[pos - 2] != 32) & (buf[pos - 3] != 32)]
        first = (-seen) % every
        sel = pos[first::every]
        seen += int(pos.numel())
        buf[sel - 1] = ord("%")
        planted += int(sel.numel())
    return planted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--percent", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch

    import bench
    import logparser_amd as lpa

    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    fmt = lpa.SYNTH_FORMATS[2]
    buf, nbytes, batches = bench.generate_to_device(lpa, torch, 2, 0, args.lines, device)
    planted = sum(plant(torch, buf, off, nb, max(1, round(100.0 / args.percent))) for off, nb in batches) \
        if args.percent > 0 else 0
    torch.cuda.synchronize()
    parser = lpa.HttpdLoglineParser(fmt, lpa.get_possible_paths(fmt), device=0)
    runs = []
    for k in range(args.warmup + args.steps):
        st = [parser.run(buf.data_ptr() + off, nb, on_device=True) for off, nb in batches]
        if k >= args.warmup:
            runs.append(st)
    last = runs[-1]
    tot = lambda key: sum(r.get(key, 0) for r in last)  # noqa: E731
    ms = [sum(r["ms_total"] for r in st) for st in runs]
    uk = [sum(r["ms_uri_kernels"] for r in st) for st in runs]
    print(json.dumps({"lib": os.path.relpath(lpa.LIB_PATH, ROOT), "lines": tot("lines"), "planted": planted, "ok": tot("ok"), "bad": tot("bad"),
                      "fallback": tot("fallback"), "uri_repair_lines": tot("uri_repair_lines"), "retries": tot("retries"),
                      "step_ms": ms, "step_ms_median": statistics.median(ms), "uri_kernels_ms": uk,
                      "uri_kernels_ms_median": statistics.median(uk),
                      "gb_per_s_median": nbytes / 1e6 / statistics.median(ms)}))


if __name__ == "__main__":
    main()
