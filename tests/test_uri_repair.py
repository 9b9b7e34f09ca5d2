"""Malformed URIs repaired on the device (lp_device.h uri_repair: the chain
HttpUriDissector.dissect runs before URI.create, :160-186), CPU part: the
emulation of the device code against the oracle.  The GPU part is
test_uri_repair_gpu.py."""
import itertools
import json
import random

import golden_check
import uri_repair_corpus as urc
from test_emu_parity import all_paths, compare

# (request URI, must be decided OK).  Required: what falls under R1-R5 of
# uri_repair_corpus and has no BAD oracle result.  Not required (FALLBACK or
# exact, never wrong): entities with another ASCII result.
PROBES = [
    ("/a?x=50%-off", True), ("/p%%%q?x=%%%3d%", True), ("/a?x=%a%a%", True), ("/a?x=1&amp;y=2", True),
    ("/a?r=A#&f=B&s=#&n=1", True), ("/a#foo#bar#baz", True), ("/a?_r=1#x3D;12&R&#x3D;E", True),
    ("/a?x=&#;1", True), ("/a?x=&#x;1", True), ("/a?x=&#xZZ;1", True), ("/a?amp;x=1", True),
    ("/a?x=1?amp;y=2", True), ("/a#?x", True), ("/a?x=1#?y", True), ("/a#x41;b?x=1", True),
    ("/a?x=&#65;&#x42;&#X43;", True), ("/a?x=&#99999999999;", True), ("/a%", True), ("/a%4", True),
    ("/a%u0041?x=%u0041", True), ("/a?x==##&y", True), ("/a b?x={%}&y=%41+b", True),
    ("http://h.example.com:80/p?x=%zz#f%", True), ("/a?x=&#38;y=2", True), ("/a?x=&#61;#b", True),
    ("/a?x=1&amp;amp;y", True), ("/a?k=#", True), ("/p?a=1&amp;b=2&amp;c=3#f#g", True), ("/a?x=1%#y%", True),
    # allowed either way (the oracle: BAD for all but the first)
    ("/a?x=&#35;frag", False), ("/a?x=&#37;zz", False), ("/a?x=&lt;", False), ("/a?x=&quot;", False),
    ("/a?x=&#32;", False),
    ("/a?x=&gt;", False), ("/a?x=&#34;", False),
]

# Required as well: an entity in place of the first '?' / '&' (it takes the
# '&' of the "?&" the reference made there: the query has no leading '&'),
# and a '&' that an entity makes before the first '?' / '&' (path text).
FIRST_SEP_PROBES = [
    "/a?#x41;b=1", "/a#x26;b?x=1", "/a?#61;b", "/a?#x3D;", "/a&#x41;b=1&c=2", "/a#x26;b", "/a#x26;b#f", "/a?#x26;b=1",
    "/a?amp;#x41;b=1", "/a#f?#x41;b", "/a#x26;#x26;b?c=%zz", "http://h.example.com/p#x26;q?#x2D;=1#g#h", "/a?#65;=#&z",
]


def _line(uri, referer="-"):
    return '1.2.3.4 - - [10/Oct/2026:13:55:36 +0200] "GET %s HTTP/1.1" 200 123 "%s" "ua"' % (uri, referer)


def test_probe_uris(oracle, emu):
    assert len(PROBES) == 36 and sum(1 for _, req in PROBES if req) == 29
    o = oracle.Oracle("combined", all_paths(oracle))
    e = emu.Emu("combined", all_paths(oracle))
    for uri, required in PROBES:
        for l in (_line(uri), _line("/ok", uri)):
            s1, r1 = o.parse_raw(l)
            s2, r2 = e.parse_raw(l)
            assert s1 != 2, l  # the oracle decides every probe
            if required:
                assert s1 == 0 and s2 == 0, (l, s1, s2)
            if s2 != 2:
                assert (s1, r1) == (s2, r2), (l, s1, s2, r1, r2)


def test_first_separator_probes(oracle, emu):
    o = oracle.Oracle("combined", all_paths(oracle))
    e = emu.Emu("combined", all_paths(oracle))
    for uri in FIRST_SEP_PROBES:
        for l in (_line(uri), _line("/ok", uri)):
            s1, r1 = o.parse_raw(l)
            s2, r2 = e.parse_raw(l)
            assert s1 in (0, 1) and (s1, r1) == (s2, r2), (l, s1, s2, r1, r2)


def test_reference_vectors_decided(emu, vectors):
    """TestHttpUriDissector.java:162-213 (bad escapes, several '#', "=#" /
    "#&", "&#x3D;" / "#x3D;"): decided on the device, with the reference's values."""
    cases = [c for c in vectors["cases"] if c["source"].startswith("hpt/dissectors/TestHttpUriDissector.java:")
             and int(c["source"].split(":")[1].split("-")[0]) >= 162]
    assert len(cases) == 7
    for c in cases:
        e = emu.Emu(c["logformat"], c["fields"], c["remaps"])
        assert e.status == 0
        st, rec = e.parse(c["line"])
        assert st != 2, c["line"]
        assert golden_check.check_case(c, st, rec or {}) == [], c["line"]


def test_in_scope_corpus(oracle, emu):
    lines = urc.in_scope(1, 3000)
    o = oracle.Oracle("combined", all_paths(oracle))
    for l in lines:
        assert o.parse_raw(l)[0] != 2, l  # a generator bug: the oracle decides every in-scope line
    e = emu.Emu("combined", all_paths(oracle))
    s = compare(o, e, lines, allow_fallback=False)
    assert s["ok"] + s["bad"] == 3000 and s["ok"] >= 2900, s


def test_out_of_scope_stays_fallback(oracle, emu):
    e = emu.Emu("combined", all_paths(oracle))
    for l in urc.out_of_scope():
        assert e.parse_raw(l)[0] == 2, l


def test_fuzz_suffixes(oracle, emu):
    """Every line the emulation decides equals the oracle (FALLBACK allowed:
    its share is printed, test_in_scope_corpus holds the zero-FALLBACK condition)."""
    alphabet = "%a4z#&=?;x"
    rng = random.Random(20261019)
    sufs = ["".join(t) for n in range(1, 5) for t in itertools.product(alphabet, repeat=n)]
    sufs += ["".join(rng.choice(alphabet) for _ in range(rng.randint(5, 12))) for _ in range(20000)]
    o = oracle.Oracle("combined", all_paths(oracle))
    e = emu.Emu("combined", all_paths(oracle))
    lines = [_line(pre + s) for s in sufs for pre in ("/p?k=", "/p")]
    s = compare(o, e, lines)
    print("fuzz: %d lines, FALLBACK share %.4f" % (len(lines), s["fallback"] / len(lines)), s)
    # that alphabet has no byte URIUtil escapes: a second one with ' ' and '{'
    # (URIUtil.encode runs before the chain in the reference, after it here)
    alphabet2 = "% {4a#&=?;x"
    sufs2 = ["".join(rng.choice(alphabet2) for _ in range(rng.randint(2, 10))) for _ in range(6000)]
    lines2 = [_line(pre + s) for s in sufs2 for pre in ("/p?k=", "/p")]
    s = compare(o, e, lines2)
    print("fuzz, escaped bytes: %d lines, FALLBACK share %.4f" % (len(lines2), s["fallback"] / len(lines2)), s)


def test_in_scope_lines_in_batch_context(oracle, emu):
    """The lines in place inside a batch buffer, at every 4-byte phase, equal
    the same lines parsed alone."""
    lines = urc.in_scope(5, 240)
    e = emu.Emu("combined", all_paths(oracle))
    alone = [e.parse_raw(l) for l in lines]
    for phase in range(4):
        data = b"p" * (phase + 4) + b"\n" + b"\n".join(lines) + b"\n"
        got = e.parse_batch_raw(data)[1:]
        assert len(got) == len(lines)
        for l, a, g in zip(lines, alone, got):
            assert a[0] in (0, 1) and a == g, (phase, l, a[0], g[0])
            assert a[0] == 1 or json.loads(g[1])
