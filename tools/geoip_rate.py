"""GeoIP lookups (k_geoip_lines, csrc/geoip.hip) beside the parse and URI
kernels of the same batch, DESIGN.md section 6.14.

    python tools/geoip_rate.py [--lines N] [--networks M] [--runs K]

One process, one build.  A large synthetic MaxMind DB is written once to a
temporary file with the tests' writer (tests/geoip_corpus.py): M random
networks (IPv4 /8../24 below ::/96, IPv6 /20../64) over 4,096 distinct City
records, ip_version 6, 32-bit records; its size and node count are recorded.
N config-2 lines (bench.py's generator and seed) are parsed by two handles:
every path of 'combined', and the same plus three City outputs.  Per handle
the HIP-event times of the batch, of the parse kernels and of the URI kernels
(lp_last_timing), and of k_geoip_lines for the second; then the device table
of three GeoIP columns beside three token columns.  config 2 holds IPv4
addresses and 5 % host names (FALLBACK under GeoIP); whether IPv4 or IPv6
texts cost more is measured on two one-token corpora ("%h") of N / 4 random
addresses each, drawn from the database's networks.  Prints one JSON line.
"""
import argparse
import ipaddress
import json
import os
import random
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEO = ["STRING:connection.client.host.country.name", "STRING:connection.client.host.city.name",
       "STRING:connection.client.host.location.latitude"]
TOKENS = ["IP:connection.client.host", "STRING:request.status.last", "BYTESCLF:response.body.bytes"]


def big_database(gc, networks, seed=20261021):
    rnd = random.Random(seed)
    w = gc.Writer(6, 32, "Synthetic-City")
    offs = [w.data(gc.city("City%d" % k, iso="C%d" % (k % 200), location={"latitude": k / 16.0 - 90, "longitude": k / 8.0 - 180}))
            for k in range(4096)]
    nets = {4: [], 6: []}
    for k in range(networks):
        if k % 4 < 3:
            plen = rnd.randrange(8, 25)
            net = ipaddress.ip_network((rnd.getrandbits(plen) << (32 - plen), plen))
        else:
            plen = rnd.randrange(20, 65)
            net = ipaddress.ip_network(((0x2 << 124) | (rnd.getrandbits(plen - 4) << (128 - plen)), plen))
        try:
            w.insert(net, rnd.choice(offs))
        except AssertionError:  # inside, or around, a network already there
            continue
        nets[net.version].append(net)
    return w.to_bytes(), len(w.nodes), nets


def address_lines(nets, n, seed):
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        net = rnd.choice(nets)
        if rnd.random() < 0.3:  # outside the networks now and then: the walk ends early
            a = ipaddress.ip_address(rnd.getrandbits(net.max_prefixlen)) if net.version == 4 else \
                ipaddress.IPv6Address((0x2 << 124) | rnd.getrandbits(124))
        else:
            a = net.network_address + rnd.randrange(net.num_addresses)
        out.append(str(a))
    return ("\n".join(out) + "\n").encode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=10_000_000)
    ap.add_argument("--networks", type=int, default=200_000)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import logparser_amd as lpa
    import bench
    import geoip_corpus as gc
    torch.cuda.set_device(0)
    data, nodes, nets = big_database(gc, args.networks)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "big.mmdb")
        with open(path, "wb") as f:
            f.write(data)
        out = {"database": {"bytes": len(data), "nodes": nodes, "record_size": 32, "ip_version": 6,
                            "tree_image_bytes": 8 * nodes + 16, "networks_v4": len(nets[4]), "networks_v6": len(nets[6])},
               "lines": args.lines}
        fields = [f for f in lpa.get_possible_paths("combined") if not f.endswith("*")]
        buf, nbytes, _ = bench.generate_to_device(lpa, torch, 2, 0, args.lines, torch.device("cuda", 0))
        out["input_bytes"] = nbytes
        results = {}
        for name, extra in (("without_geoip", []), ("with_geoip", GEO)):
            p = lpa.HttpdLoglineParser("combined", fields + extra)
            if extra:
                p.add_dissector("GeoIPCityDissector", path)
            runs = []
            for _ in range(args.runs + 1):
                st = p.run(buf.data_ptr(), nbytes)
                r = lpa.BatchResult(p)
                runs.append({"ms_total": round(st["ms_total"], 3), "ms_parse_kernels": round(st["ms_parse_kernels"], 3),
                             "ms_uri_and_geoip_kernels": round(st["ms_uri_kernels"], 3), "ms_geoip": round(r.geoip_timing(), 3)})
            assert p.device_program_ok, p.unsupported_reason
            results[name] = {"ok": st["ok"], "bad": st["bad"], "fallback": st["fallback"], "runs": runs[1:]}
            # the table: three GeoIP columns / three token columns of this batch
            cols = [(c, str) for c in (extra or TOKENS)]
            first = r.table_device(cols)
            caps = {k: int(v[0][1].numel()) + 16 for k, v in first.items()}
            valid = {k: int(v[1].sum().item()) for k, v in first.items()}
            del first
            bufs = r.table_buffers(cols, chars_cap=caps)
            truns = []
            for _ in range(args.runs):
                r.table_device(cols, buffers=bufs)
                t = r.table_timing()
                truns.append({k: round(v, 3) for k, v in t.items()} | {"total": round(sum(t.values()), 3)})
            results[name]["table"] = {"columns": [c for c, _ in cols], "valid_rows": valid, "ms": truns}
            del bufs, r, p
            torch.cuda.empty_cache()
        out.update(results)
        g = min(x["ms_geoip"] for x in results["with_geoip"]["runs"])
        tot = min(x["ms_total"] for x in results["with_geoip"]["runs"])
        base = min(x["ms_total"] for x in results["without_geoip"]["runs"])
        out["geoip_share_of_batch"] = round(g / tot, 4)
        out["batch_ms_with_over_without"] = round(tot / base, 4)
        out["geoip_lookups_per_s"] = round(args.lines / (g / 1e3)) if g > 0 else None
        del buf
        # IPv4 against IPv6 texts: one-token lines, the same database
        fam = {}
        for v in (4, 6):
            lines = address_lines(nets[v], max(1, args.lines // 4), 7 + v)
            t = torch.frombuffer(bytearray(lines), dtype=torch.uint8).cuda()
            p = lpa.HttpdLoglineParser("%h", GEO).add_dissector("GeoIPCityDissector", path)
            ms = []
            for _ in range(args.runs + 1):
                st = p.run(t.data_ptr(), len(lines))
                ms.append(round(lpa.BatchResult(p).geoip_timing(), 3))
            r = lpa.BatchResult(p)
            found = int(r.table_device([(GEO[0], str)])[GEO[0]][1].sum().item())
            n = lines.count(b"\n")
            fam["ipv%d" % v] = {"lines": n, "bytes": len(lines), "ok": st["ok"], "fallback": st["fallback"], "found": found,
                                "ms_geoip": ms[1:], "ns_per_line": round(min(ms[1:]) * 1e6 / n, 3),
                                "ms_parse_kernels": round(st["ms_parse_kernels"], 3)}
            del t, p, r
        out["by_family"] = fam
    print(json.dumps(out))


if __name__ == "__main__":
    main()
