"""IPv6 client addresses in FORMAT_IP / FORMAT_CLF_IP tokens (TokenParser.java:43-52)
decided on the device by match_line (ip_resolve): a sole end of the token that
the format's next literal follows is the token's candidate, several such ends
are resolved by a nested DFS (exactly one completes: that one; two or more:
FALLBACK).  The chunk kernel queues these lines for the overflow kernels
(the sole-end walk inside the first leaf cost config 5
more than the parent's run-to-run spread), diag["dfs_lines"] counts them.  CPU tests run the emulation of
lp_device.h (both LineT flavours), GPU tests the kernels, both against the
oracle."""
import json
import random
import time

import pytest

import logparser_amd as lpa
from test_emu_parity import IP_TOKENS, MIXED, NGINX, compare

APACHE_IP = '%a %l %u %t "%r" %>s %b'

# the addresses of the issue's list, then the further ones of its test 1
V6_HOSTS = ["2001:db8::1", "fe80::1", "::1", "::", "2001:0db8:85a3:0000:0000:8a2e:0370:7334", "::ffff:192.0.2.128",
            "64:ff9b::192.0.2.33", "FE80::ABCD", "1::", "2001:db8:0:0:1:0:0:1", "abcd:ef01:2345:6789:abcd:ef01:2345:6789"]
HOSTS = V6_HOSTS + ["192.0.2.77", "-"]

ODD_TOKENS = [b"::1 ", b"dead:beef cafe", b"2001:db8:::1", b"12345::1", b"a:b:c:d:e:f:1:2:3", b"2001:db8::1%eth0",
              b"[::1]", b"1:2\xc3\xa9"]

TIER2_HOSTS = [b"dead beef", b"a b", b"cafe f00d"]
APACHE_TAIL = b' [10/Oct/2000:13:55:36 -0700] "GET /apache_pb.gif?x=1 HTTP/1.0" 200 2326'

_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def swap_host(line, host):
    if isinstance(host, str):
        host = host.encode()
    return host + line[line.index(b" "):]


def nginx_base(n):
    return cached(("nginx", n), lambda: lpa.synth(lpa.SYNTH_NGINX, 20261019, 0, n).split(b"\n")[:-1])


def mixed_base(n):
    return cached(("mixed", n), lambda: lpa.synth(lpa.SYNTH_MIXED, 20261019, 0, n).split(b"\n")[:-1])


def apache_ip_lines(hosts):
    """'%a %l %u %t "%r" %>s %b' lines built by hand, two users for each host"""
    return [(h.encode() if isinstance(h, str) else h) + b" - " + u + APACHE_TAIL for h in hosts for u in (b"frank", b"-")]


def odd_lines():
    """test 2's lines: IP_TOKENS and ODD_TOKENS in front of ten NGINX base lines"""
    toks = [t.encode() for t in IP_TOKENS] + ODD_TOKENS
    return [swap_host(l, t) for l in nginx_base(600)[:10] for t in toks]


def tier2_lines():
    return [h + b" - " + u + APACHE_TAIL for h in TIER2_HOSTS for u in (b"frank", b"-")]


def oracle_pair(oracle, emu, fmt):
    paths = cached(("paths", fmt), lambda: oracle.possible_paths(fmt))
    e = emu.Emu(fmt, paths)
    assert e.status == 0, e.err
    return oracle.Oracle(fmt, paths), e


def host_of(record_json):
    """the IP token's value ($remote_addr: connection.client.host, %a: connection.client.ip)"""
    rec = json.loads(record_json)
    v = rec["IP:connection.client.host"] if "IP:connection.client.host" in rec else rec["IP:connection.client.ip"]
    assert len(v) == 1
    return v[0]


# ------------------------------------------------------------------ CPU (emulation)

def test_wellformed_ipv6_hosts_emulated(oracle, emu):
    """Test 1.  Well-formed IPv6 hosts (and an IPv4 host and '-') as the first
    token of 600 NGINX config-4 lines, of 600 lines of the three-format MIXED
    corpus, and of hand-built '%a ...' lines: every line OK with the oracle's
    record, none FALLBACK."""
    for fmt, base in ((NGINX, nginx_base(600)), (MIXED, mixed_base(600))):
        o, e = oracle_pair(oracle, emu, fmt)
        lines = [swap_host(l, HOSTS[i % len(HOSTS)]) for i, l in enumerate(base)]
        s = compare(o, e, lines, allow_fallback=False)
        assert s["ok"] == len(lines), (fmt[:20], s)
    o, e = oracle_pair(oracle, emu, APACHE_IP)
    lines = apache_ip_lines(HOSTS)
    s = compare(o, e, lines, allow_fallback=False)
    assert s["ok"] == len(lines) == 26, s
    for l in lines[:2 * len(V6_HOSTS)]:
        assert host_of(e.parse_raw(l)[1]) == l.split(b" ")[0].decode()


def test_odd_ip_tokens_emulated(oracle, emu):
    """Test 2.  Odd first tokens before the NGINX literal ' - ': at most one
    end of the token is followed by it, so every line is decided as the
    oracle decides it (status, and the record when OK), none FALLBACK."""
    o, e = oracle_pair(oracle, emu, NGINX)
    base = nginx_base(600)[:10]
    assert compare(o, e, base, allow_fallback=False)["ok"] == len(base)  # (OK with their IPv4 hosts)
    lines = odd_lines()
    s = compare(o, e, lines, allow_fallback=False)
    assert s["fallback"] == 0 and s["ok"] + s["bad"] == len(lines), s
    # what the oracle says of the added tokens: OK with the whole token for the first five
    for t in ODD_TOKENS[:5]:
        st, js = o.parse_raw(swap_host(base[0], t))
        assert st == oracle.OK and host_of(js) == t.decode(), t
    for t in ODD_TOKENS[5:7]:
        assert o.parse_raw(swap_host(base[0], t))[0] == oracle.BAD, t


TWO_ENDS_FMT = "%a %{Foo}i"
TWO_ENDS_LINE = b"dead beef cafe"


def test_several_ends_tier2_emulated(oracle, emu):
    """Test 3.  '%a' before the literal ' ' with a host of two hex words:
    two ends of the token are followed by ' ', and only the longer one lets
    '%l %u %t' match: the nested DFS finds it, the record is the oracle's.
    Two completing ends: '%a %{Foo}i' on 'dead beef cafe' reads as
    (dead | beef cafe) and as (dead beef | cafe); the oracle shows each
    reading with the other one's second word pinned by a literal.  The device
    models no priority among them: FALLBACK."""
    o, e = oracle_pair(oracle, emu, APACHE_IP)
    lines = tier2_lines()
    s = compare(o, e, lines, allow_fallback=False)
    assert s["ok"] == len(lines), s
    for l in lines:
        assert host_of(e.parse_raw(l)[1]) == b" ".join(l.split(b" ")[:2]).decode()
    for fmt, want in (("%a beef %{Foo}i", "dead"), ("%a cafe", "dead beef")):
        st, js = oracle.Oracle(fmt, ["IP:connection.client.ip"]).parse_raw(TWO_ENDS_LINE)
        assert st == oracle.OK and host_of(js) == want, (fmt, st, js)
    o2, e2 = oracle_pair(oracle, emu, TWO_ENDS_FMT)
    assert o2.parse_raw(TWO_ENDS_LINE)[0] == oracle.OK
    assert e2.parse_raw(TWO_ENDS_LINE)[0] == 2
    # one word: a sole end again
    assert compare(o2, e2, [b"dead beef", b"::1 x y"], allow_fallback=False)["ok"] == 2


def test_hostile_hosts_keep_the_budget_emulated(oracle, emu):
    """Test 4.  Hosts of 4,000 bytes ('a:' and 'a ' repeated): the oracle's
    status or FALLBACK, and promptly (the nested runs share the line's step
    budget of 16 n + 256 element visits: a second is ample for it)."""
    for fmt in (NGINX, APACHE_IP):
        o, e = oracle_pair(oracle, emu, fmt)
        for unit in (b"a:", b"a "):
            host = unit * 2000
            tail = nginx_base(600)[0] if fmt == NGINX else b"1.2.3.4 - frank" + APACHE_TAIL
            line = swap_host(tail, host)
            t0 = time.perf_counter()
            st = e.parse_raw(line)[0]
            dt = time.perf_counter() - t0
            print("host %r x 2000, %s: status %d in %.4f s" % (unit, fmt[:12], st, dt))
            assert st in (o.parse_raw(line)[0], 2), (fmt[:12], unit, st)
            assert dt < 1.0, dt


# ------------------------------------------------------------------ GPU

def ipv6_corpus(base, seed, only=None):
    """30 % of the lines (of those `only` accepts) get an IPv6 host, fixed seed.  Returns (lines, indices)."""
    rng = random.Random(seed)
    out, v6 = [], []
    for i, l in enumerate(base):
        if (only is None or only(l)) and rng.random() < 0.3:
            out.append(swap_host(l, rng.choice(V6_HOSTS)))
            v6.append(i)
        else:
            out.append(l)
    return out, v6


def config4_batch(oracle):
    """test 5's batch (shared with test 8): (lines, IPv6 line indices, stats, result)"""
    def make():
        from test_gpu_parity import gpu_vs_oracle, paths
        lines, v6 = ipv6_corpus(lpa.synth(lpa.SYNTH_NGINX, 20261020, 0, 4000).split(b"\n")[:-1], 61)
        s, r = gpu_vs_oracle(oracle, NGINX, paths(oracle, NGINX), lines, allow_fallback=False)
        return lines, v6, s, r
    return cached("config4_batch", make)


@pytest.mark.gpu
def test_config4_ipv6_corpus_gpu(oracle):
    """Test 5.  4,000 config-4 lines, 30 % with IPv6 hosts: every line OK and
    its record the oracle's (gpu_vs_oracle compares all 4,000); the IPv6 lines,
    and only they, are queued for the DFS (tier 1 sits behind the queue:
    DESIGN.md section 6.1), and the same statuses and records from HBM
    (LP_OPT_FORCE_DIRECT: the SWAR LineT)."""
    from test_gpu_parity import paths
    lines, v6, s, r = config4_batch(oracle)
    assert 1000 < len(v6) < 1400
    assert s["ok"] == 4000, s
    assert r.diag["dfs_lines"] == len(v6), (r.diag, len(v6))
    recs = [r.record_json(i) for i in range(4000)]
    for i in v6:
        assert host_of(recs[i]) == lines[i].split(b" ")[0].decode()
    p = lpa.HttpdLoglineParser(NGINX, paths(oracle, NGINX), options={lpa.OPT_FORCE_DIRECT: 1})
    rd = p.parse_batch(b"".join(l + b"\n" for l in lines))
    assert rd.n_lines == 4000 and (rd.status == lpa.LINE_OK).all()
    assert [rd.record_json(i) for i in range(4000)] == recs


@pytest.mark.gpu
def test_mixed_handle_ipv6_gpu(oracle):
    """Test 6.  4,000 lines of the three-format corpus, IPv6 hosts on 30 % of
    the NGINX ones, line by line against the sticky oracle: no FALLBACK."""
    from test_gpu_parity import paths
    base = lpa.synth(lpa.SYNTH_MIXED, 20261021, 0, 4000).split(b"\n")[:-1]
    lines, v6 = ipv6_corpus(base, 62, only=lambda l: not l.endswith(b'"') and l[-1:] in (b"p", b"."))
    assert len(v6) > 250
    fields = paths(oracle, MIXED)
    r = lpa.HttpdLoglineParser(MIXED, fields).parse_batch(b"".join(l + b"\n" for l in lines))
    assert r.n_lines == 4000

    def want():
        o = oracle.Oracle(MIXED, fields)
        return [o.parse_raw(l) for l in lines]
    for i, (s1, r1) in enumerate(cached("mixed_oracle", want)):
        s2 = int(r.status[i])
        assert s2 != lpa.LINE_FALLBACK, (i, lines[i])
        assert s1 == s2, (i, lines[i], s1, s2)
        if s1 == oracle.OK:
            assert r1 == r.record_json(i), (i, lines[i])
    assert r.counters["fallback"] == 0 and r.counters["ok"] == 4000, r.counters


@pytest.mark.gpu
def test_odd_and_tier2_lines_gpu(oracle, emu):
    """Test 7.  The lines of tests 2 and 3 on the GPU (k_parse_ovf_lines for
    the ones the first leaf does not decide): the statuses, records and
    FALLBACK count of the CPU emulation."""
    from test_gpu_parity import paths
    for fmt, lines in ((NGINX, odd_lines()), (APACHE_IP, tier2_lines()), (TWO_ENDS_FMT, [TWO_ENDS_LINE, b"dead beef"])):
        fields = paths(oracle, fmt)
        e = emu.Emu(fmt, fields)
        r = lpa.HttpdLoglineParser(fmt, fields).parse_batch(b"".join(l + b"\n" for l in lines))
        assert r.n_lines == len(lines)
        fb = 0
        for i, l in enumerate(lines):
            st, js = e.parse_raw(l)
            assert int(r.status[i]) == st, (fmt[:12], l, st, int(r.status[i]))
            if st == 0:
                assert r.record_json(i) == js, (fmt[:12], l)
            fb += st == 2
        assert r.counters["fallback"] == fb, (r.counters, fb)
        if fmt == TWO_ENDS_FMT:
            assert fb == 1
        else:
            assert fb == 0


@pytest.mark.gpu
def test_device_table_ipv6_hosts_gpu(oracle):
    """Test 8.  The device table's STRING column of IP:connection.client.host
    on test 5's batch holds the oracle's values (the IPv6 spans through
    table.hip), null where the host is '-'."""
    from test_gpu_parity import paths
    lines, v6, _, r = config4_batch(oracle)
    path = "IP:connection.client.host"
    (off, chars), valid = r.table_device([(path, str)])[path]
    off, chars, valid = off.cpu().numpy(), chars.cpu().numpy().tobytes(), valid.cpu().numpy().astype(bool)
    o = oracle.Oracle(NGINX, [path])
    for i, l in enumerate(lines):
        st, js = o.parse_raw(l)
        assert st == oracle.OK
        v = host_of(js)
        if v is None:
            assert not valid[i], (i, l)
        else:
            assert valid[i] and chars[off[i]:off[i + 1]].decode() == v, (i, l)
    assert sum(1 for i in v6 if b":" in chars[off[i]:off[i + 1]]) == len(v6)
