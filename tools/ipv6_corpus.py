"""Throughput of a config-4 (NGINX) corpus whose hosts are partly IPv6, next to
the IPv4-only corpus: lp_synth workload 4 lines, the first token of a share of
them rewritten on the host (fixed seed), parsed from device memory.
Usage: ipv6_corpus.py [LINES] [SHARE, percent]."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import logparser_amd as lpa  # noqa: E402

V6 = [b"2001:db8::1", b"fe80::1", b"::1", b"::", b"2001:0db8:85a3:0000:0000:8a2e:0370:7334", b"::ffff:192.0.2.128",
      b"64:ff9b::192.0.2.33", b"FE80::ABCD", b"1::", b"2001:db8:0:0:1:0:0:1", b"abcd:ef01:2345:6789:abcd:ef01:2345:6789"]

n = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
share = float(sys.argv[2]) / 100.0 if len(sys.argv) > 2 else 0.3
fmt = lpa.SYNTH_FORMATS[lpa.SYNTH_NGINX]
fields = lpa.get_possible_paths(fmt)
base = lpa.synth(lpa.SYNTH_NGINX, 20261017, 0, n)
rng = random.Random(20261019)
lines = base.split(b"\n")
n6 = 0
for i in range(n):
    if rng.random() < share:
        l = lines[i]
        lines[i] = rng.choice(V6) + l[l.index(b" "):]
        n6 += 1
mixed = b"\n".join(lines)
for name, data, want6 in (("IPv4 only", base, 0), ("%.0f %% IPv6" % (100 * share), mixed, n6)):
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    p = lpa.HttpdLoglineParser(fmt, fields)
    for _ in range(2):
        p.run(t.data_ptr(), len(data))
    tot, ks = [], []
    for _ in range(5):
        st = p.run(t.data_ptr(), len(data))
        tot.append(st["ms_total"])
        ks.append(st["ms_parse_kernels"])
    ms = sorted(tot)[2]
    print("%-12s %d lines (%d IPv6), %.1f MB: median %.3f ms = %.1f GB/s, parse kernels %.3f ms; ok %d bad %d "
          "fallback %d queued %d of them for the DFS %d" %
          (name, n, want6, len(data) / 1e6, ms, len(data) / ms / 1e6, sorted(ks)[2], st["ok"], st["bad"], st["fallback"],
           st["overflow_waves"], st["dfs_lines"]), flush=True)
