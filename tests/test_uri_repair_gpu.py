"""Malformed URIs repaired on the device, GPU part: k_uri_lines queues the
lines whose URI the reference repairs before URI.create, k_uri_overflow
redoes their phase 2 and that of such lines of its own waves (uri.hip
uri_redo_line, lp_device.h uri_repair).
The CPU part (the emulation of the same code) is test_uri_repair.py."""
import random
import re

import numpy as np
import pytest

import logparser_amd as lpa
import uri_repair_corpus as urc
from test_gpu_parity import _device_vs_host_table, expected_histograms, gpu_vs_oracle, paths

pytestmark = pytest.mark.gpu


def _decided(oracle, lines, options=None, fmt="combined"):
    """every line equals the oracle, none is FALLBACK, the counters equal the
    per-line statuses (gpu_vs_oracle); returns the result"""
    if options is None:
        s, r = gpu_vs_oracle(oracle, fmt, paths(oracle, fmt), lines, allow_fallback=False)
    else:
        fields = paths(oracle, fmt)
        p = lpa.HttpdLoglineParser(fmt, fields, options=options)
        r = p.parse_batch(b"".join(l + b"\n" for l in lines))
        o = oracle.Oracle(fmt, fields)
        s = {"ok": 0, "bad": 0, "fallback": 0}
        for i, l in enumerate(lines):
            s1, r1 = o.parse_raw(l)
            assert s1 == int(r.status[i]) and s1 != oracle.UNSUPPORTED, (i, l, s1, int(r.status[i]))
            if s1 == oracle.OK:
                assert r1 == r.record_json(i), (i, l)
            s["ok" if s1 == oracle.OK else "bad"] += 1
        c = r.counters
        assert (c["lines"], c["ok"], c["bad"], c["fallback"]) == (len(lines), s["ok"], s["bad"], 0), c
    assert s["fallback"] == 0 and r.counters["fallback"] == 0
    return r


def test_in_scope_corpus_gpu(oracle):
    lines = urc.in_scope(2, 8192)
    r = _decided(oracle, lines)
    assert r.diag["uri_repair_lines"] >= len(lines), r.diag  # every request URI carries a defect
    assert r.counters["ok"] >= 8000, r.counters


@pytest.mark.parametrize("n, defective", [(1, "all"), (64, "all"), (65, "all"), (130, "all"), (130, "none"),
                                          (130, "edges")])
def test_queue_geometry_gpu(oracle, n, defective):
    """The queue holds every line of the batch, none, or lines 0, 63, 64 and
    the last (the first and last lanes of two waves)."""
    rng = random.Random(n)
    which = {"all": set(range(n)), "none": set(), "edges": {0, 63, 64, n - 1}}[defective]
    lines = [urc.in_scope_line(rng, k, referer="-") if k in which else urc.clean_line(rng, k) for k in range(n)]
    r = _decided(oracle, lines)
    assert r.diag["uri_repair_lines"] == len(which), r.diag


def test_both_stages_and_second_only_gpu(oracle):
    """Both URI stages of a line defective, and only the second (the referer):
    the redo rewrites the request URI's values too, and they equal the oracle's."""
    rng = random.Random(33)
    lines = []
    for k in range(192):
        ref = urc.plant(rng, urc.clean_uri(rng, absolute=True), urc.CLASSES[k % 6])
        if k % 2:
            lines.append(urc.in_scope_line(rng, k, referer=ref))
        else:
            lines.append(urc.line(rng, k, urc.clean_uri(rng), ref))
    r = _decided(oracle, lines)
    assert r.diag["uri_repair_lines"] == len(lines), r.diag
    assert r.counters["ok"] >= 180, r.counters


@pytest.mark.parametrize("direct", [0, 1])
def test_long_defective_uris_gpu(oracle, direct):
    """Defective URIs in a wave whose URI bytes exceed the URI kernel's compact
    buffer (the wave runs in k_uri_overflow: the second wave here, and one
    line of 6 KiB in the first) and in one exceeding that kernel's buffer too
    (the third: the lines' bytes read from HBM); also with every parse wave on
    the direct path.  (A line longer than MAX_LINE is FALLBACK in phase 1.)"""
    rng = random.Random(44)
    lines = [urc.clean_line(rng, k) for k in range(192)]
    want = 0
    for k in range(192):
        size = 6000 if k == 5 else 0 if k < 64 else 300 if k < 128 else 700
        if not size:
            continue
        uri = "/long/p%41th?" + "&".join("k%d=v%d" % (j, j) for j in range(size // 6))[:size]
        if k % 4 == 1:
            uri += "&x=50%-off&amp;y=#&z=1#a#b"
            want += 1
        lines[k] = urc.line(rng, k, uri, "http://www.example.com/r?x=%zz" if k % 8 == 1 else "-")
    r = _decided(oracle, lines, options={lpa.OPT_FORCE_DIRECT: direct})
    assert r.diag["uri_repair_lines"] == want and r.diag["uri_overflow_waves"] >= 2, r.diag
    assert r.counters["ok"] == 192, r.counters


def test_three_formats_gpu(oracle):
    """The formats and corpus of test_mixed_formats_gpu, defects planted in
    request URIs of every format (the 'combined' and NGINX ones among them)."""
    from test_emu_parity import MIXED, mixed_lines
    fields = paths(oracle, MIXED)
    rng = random.Random(61)
    req = re.compile(rb'"([A-Z]+) (\S+) (HTTP/[0-9.]+)"')
    lines, planted = [], set()
    for k, l in enumerate(mixed_lines(4096, 62)):
        m = req.search(l)
        if m and k % 3 == 0:
            uri = urc.plant(rng, m.group(2).decode("ascii"), urc.CLASSES[(k // 3) % 6]).encode("ascii")
            l = l[:m.start(2)] + uri + l[m.end(2):]
            planted.add(k)
        lines.append(l)
    assert len(planted) > 1000
    p = lpa.HttpdLoglineParser(MIXED, fields)
    r = p.parse_batch(b"".join(l + b"\n" for l in lines))
    o = oracle.Oracle(MIXED, fields)
    ok = 0
    for i, l in enumerate(lines):
        s1, r1 = o.parse_raw(l)  # (stateful: every line, in order)
        s2 = int(r.status[i])
        if s2 == lpa.LINE_FALLBACK:
            assert i not in planted, (i, l)
            continue
        assert s1 == s2, (i, l, s1, s2)
        if s1 == oracle.OK:
            assert r1 == r.record_json(i), (i, l)
            ok += 1
    assert ok > 0.9 * len(lines)
    # (a planted line that is BAD in phase 1 never reaches the URI kernels)
    assert r.diag["uri_repair_lines"] >= sum(1 for i in planted if int(r.status[i]) == lpa.LINE_OK) > 1300, r.diag


def test_short_arena_gpu(oracle):
    """A far too small first arena: the batch re-runs (the repair kernel's
    regions and spills count towards the next estimate) and ends equal to the
    oracle; lines may only differ as FALLBACK with arena_ovf left > 0."""
    lines = urc.in_scope(3, 4096)
    fields = paths(oracle)
    p = lpa.HttpdLoglineParser("combined", fields, reserve_arena=4096, options={lpa.OPT_ARENA_BYTES: 64 * 1024})
    r = p.parse_batch(b"".join(l + b"\n" for l in lines))
    assert r.diag["retries"] > 0, r.diag
    o = oracle.Oracle("combined", fields)
    fb = 0
    for i, l in enumerate(lines):
        s1, r1 = o.parse_raw(l)
        if int(r.status[i]) == lpa.LINE_FALLBACK:
            fb += 1
            continue
        assert s1 == int(r.status[i]), (i, l)
        if s1 == oracle.OK:
            assert r1 == r.record_json(i), (i, l)
    print("short arena: retries %d, arena_ovf %d, FALLBACK %d" % (r.diag["retries"], r.diag["arena_ovf"], fb))
    assert fb == 0 or r.diag["arena_ovf"] > 0, (fb, r.diag)
    assert r.counters["fallback"] == fb


def test_device_table_gpu(oracle):
    """lp_result_table on the device equals the host table where the parts of
    a URI are refs into the repaired copy in the line's region."""
    lines = urc.in_scope(4, 4096)
    fields = lpa.get_possible_paths("combined")
    p = lpa.HttpdLoglineParser("combined", fields)
    r = p.parse_batch(b"".join(l + b"\n" for l in lines))
    assert r.counters["fallback"] == 0 and r.diag["uri_repair_lines"] >= 4096, (r.counters, r.diag)
    _, res = r.copy_to_host()
    names = ["HTTP.PATH:request.firstline.uri.path", "HTTP.QUERYSTRING:request.firstline.uri.query",
             "HTTP.REF:request.firstline.uri.ref", "HTTP.PATH:request.referer.path",
             "HTTP.QUERYSTRING:request.referer.query", "HTTP.REF:request.referer.ref",
             "STRING:request.firstline.uri.query.a", "STRING:request.firstline.uri.query.x",
             "HTTP.HOST:request.referer.host", "HTTP.PORT:request.referer.port"]
    cols = []
    for f in names:
        cols.append((f, str))
        if (p.get_casts(f) or 0) & lpa.CAST_LONG:
            cols.append((f, int))
    assert _device_vs_host_table(r, res, cols) == []


def test_histograms_gpu(oracle):
    """lp_histograms on a corpus with one third in-scope lines equals the
    counts restated from the per-line results."""
    rng = random.Random(71)
    lines = lpa.synth_combined(20261021, 0, 3000).split(b"\n")[:-1]
    lines = [urc.in_scope_line(rng, i) if i % 3 == 0 else l for i, l in enumerate(lines)]
    p = lpa.HttpdLoglineParser("combined", paths(oracle))
    r = p.parse_batch(b"".join(l + b"\n" for l in lines))
    assert r.counters["fallback"] == 0 and r.diag["uri_repair_lines"] >= 1000, (r.counters, r.diag)
    got = np.array(p.histograms(), dtype=np.int64)
    want = expected_histograms(p, r, lines, lambda i: r.record(i))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(w), int(got[w]), int(want[w])) for w in bad[:20]]
