"""Boundary corpora of the URI kernels' wave-cooperative code
(uri_wave_corpus), GPU part: the block gather of uri_compact, the three path
tiers (compact buffer, k_uri_overflow's buffer, HBM), uri_walk_coop and the
spread query-piece pass of uri_wave (uri.hip), every line against the oracle,
bit-exact.  No line may be FALLBACK, the counters equal the per-line
statuses, arena_ovf is 0, uri_repair_lines equals the planted defects.
The CPU part (the serial code on the same corpora, and the corpora's
self-checks) is test_uri_wave.py."""
import functools

import numpy as np
import pytest

import logparser_amd as lpa
import uri_wave_corpus as uwc
from test_gpu_parity import _device_vs_host_table, gpu_vs_oracle, paths
from test_uri_repair_gpu import _decided
from test_uri_wave import FMTS

pytestmark = pytest.mark.gpu

_REF = {}  # (case name, fields) -> the oracle's [(status, json)]: computed once, never changed


def _reference(oracle, case, fields):
    key = (case.name, len(case.lines), tuple(fields))
    if key not in _REF:
        o = oracle.Oracle(FMTS[case.fmt], fields)
        _REF[key] = [o.parse_raw(l) for l in case.lines]  # (stateful: every line, in order)
    return _REF[key]


def _diag(case, r):
    assert r.diag["arena_ovf"] == 0, (case.name, r.diag)
    assert r.diag["uri_repair_lines"] == len(case.defective), (case.name, r.diag, len(case.defective))
    return r


def decided(oracle, case, options=None):
    """_decided (every line equals the oracle, none FALLBACK, the counters
    equal the statuses) plus the diag conditions"""
    return _diag(case, _decided(oracle, case.lines, options, FMTS[case.fmt]))


def decided_with(oracle, case, parser, data=None):
    """the same conditions for a given parser (its fields, its options, a
    reused handle) and buffer, against the shared reference"""
    ref = _reference(oracle, case, parser.fields)
    r = parser.parse_batch(case.data if data is None else data)
    assert r.n_lines == len(case.lines), (case.name, r.n_lines)
    n = [0, 0]
    for i, (s1, r1) in enumerate(ref):
        assert s1 in (oracle.OK, oracle.BAD) and s1 == int(r.status[i]), (case.name, i, case.lines[i], s1, int(r.status[i]))
        if s1 == oracle.OK:
            assert r1 == r.record_json(i), (case.name, i, case.lines[i])
        n[s1] += 1
    c = r.counters
    assert (c["lines"], c["ok"], c["bad"], c["fallback"]) == (len(case.lines), n[0], n[1], 0), (case.name, c)
    return _diag(case, r)


def _parser(oracle, case, fields=None, options=None):
    return lpa.HttpdLoglineParser(FMTS[case.fmt], fields or paths(oracle, FMTS[case.fmt]), options=options)


# ---------------------------------------------------------------- A: gather
def test_gather_geometry_gpu(oracle):
    """A1: the request URI at every start x end offset mod 16; spans of 1, 16
    (one aligned block) and 17 bytes."""
    c = uwc.gather_geometry()
    s, r = gpu_vs_oracle(oracle, "combined", paths(oracle), c.lines, allow_fallback=False, data=c.data)
    assert s == {"ok": len(c.lines), "bad": 0, "fallback": 0}
    _diag(c, r)


def test_gather_geometry_skewed_views_gpu(oracle):
    """A4: the same buffer as a view at byte skews 1..15 of a device tensor."""
    import torch
    c = uwc.gather_geometry()
    p = _parser(oracle, c)
    data = c.data
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    for skew in range(1, 16):
        u = torch.full((len(data) + 32,), 0x26, dtype=torch.uint8, device="cuda")  # '&' around the view
        u[skew:skew + len(data)].copy_(t)
        decided_with(oracle, c, p, data=u[skew:skew + len(data)])


def test_sparse_waves_gpu(oracle):
    """A2: only lane 0 / lane 63 / alternating lanes with a URI, 40 empty
    lanes between full ones, no lane at all (block total 0)."""
    for c in uwc.sparse_waves():
        r = decided(oracle, c)
        assert r.counters["bad"] == len(c.bad) and r.diag["uri_overflow_waves"] == 0


def test_partial_last_block_gpu(oracle):
    """A3: a URI in the last, partial 16-byte block of the input, for every
    nbytes % 16 (the last line unterminated)."""
    p = None
    for c in uwc.partial_last_block():
        p = p or _parser(oracle, c)
        r = decided_with(oracle, c, p)
        assert r.counters["ok"] == 6


# ------------------------------------------------------------ B: path tiers
@functools.lru_cache(None)
def _first_tier_boundary():
    """T1: the smallest URI byte total (in 16-byte blocks) at which a wave of
    wave_with_total leaves the compact buffer, located by bisection on
    diag["uri_overflow_waves"] (monotone in T).  The counter only says where
    to test, never whether a result is right."""
    p = lpa.HttpdLoglineParser("combined", ["HTTP.QUERYSTRING:request.firstline.uri.query"])
    seen = {}

    def over(T):
        seen[T] = p.parse_batch(uwc.wave_with_total(T).data).diag["uri_overflow_waves"]
        return seen[T]

    lo, hi = 1024, 64 * 600
    assert over(lo) == 0 and over(hi) == 1, seen
    while hi - lo > 16:
        mid = (lo + hi) // 32 * 16
        if over(mid):
            hi = mid
        else:
            lo = mid
    print("tier boundary: T1 = %d bytes (%d blocks); probes %s" % (hi, hi // 16, sorted(seen.items())))
    return hi


def _tier_totals(T1):
    r16 = lambda x: int(x) // 16 * 16
    out = [T1 + 16 * d for d in range(-3, 4)]
    out += [T1 * k + d for k in (2, 3, 4, 5, 8) for d in (-16, 16)]
    out += [r16(T1 * k) for k in (1.5, 3.9, 4.1)]
    return out


def test_path_tiers_gpu(oracle):
    """B: one wave at every block around the first tier boundary, and at
    multiples of it that bracket the second (the 4x buffer of k_uri_overflow,
    then HBM)."""
    T1 = _first_tier_boundary()
    seen = {}
    for T in _tier_totals(T1):
        c = uwc.wave_with_total(T)
        r = decided(oracle, c)
        assert r.counters["ok"] == 64
        seen[T] = r.diag["uri_overflow_waves"]
    print("T1 = %d; uri_overflow_waves by T: %s" % (T1, sorted(seen.items())))


@pytest.mark.parametrize("variant", ["long", "defect"])
def test_path_tier_variants_gpu(oracle, variant):
    """B: one URI of 6400 bytes among 63 short ones; an R1 defect in lanes 0,
    31 and 63 -- one block below and above the first tier boundary."""
    T1 = _first_tier_boundary()
    for T in (T1 - 16, T1 + 16):
        c = uwc.wave_with_total(T, variant)
        r = decided(oracle, c)
        print("%s: uri_overflow_waves %d, uri_repair_lines %d" % (c.name, r.diag["uri_overflow_waves"],
                                                                 r.diag["uri_repair_lines"]))


# ------------------------------------------------- C: list / pair tokens (lin)
@pytest.mark.parametrize("kind", ["cookie", "upstream"])
def test_list_and_pair_tokens_gpu(oracle, kind):
    """C: the URIs alone take about half the compact buffer; the Cookie header
    / $upstream_addr list grows until URI and token blocks no longer fit
    together (the tokens are then read from HBM).  Which side of that a wave
    is on is not observable: only that the URIs alone always fit."""
    total = _first_tier_boundary() // 2 // 64 * 64
    make = uwc.cookie_wave if kind == "cookie" else uwc.upstream_wave
    for n in range(16, 137, 8):
        c = make(total, n)
        r = decided(oracle, c)
        assert r.counters["ok"] == 64 and r.diag["uri_overflow_waves"] == 0, (c.name, r.diag)


# ------------------------------------------------------ D: cooperative walk
@functools.lru_cache(None)
def _walk_cases():
    return {c.name: c for c in uwc.walk_cases()}


WALK_NAMES = ["D1-req", "D1-ref", "D1-both", "D2", "D3-req", "D3-ref", "D3-both", "D4-req", "D4-ref"]


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("name", WALK_NAMES)
def test_cooperative_walk_gpu(oracle, name, direct):
    """D1: lines of 0..200 events starting at every position of a 64-event
    round; D2: wave totals 63..65, 127..129; D3: every event of the PLACED
    URIs as the last event of a round and the first of the next; D4: runs of
    130 '&' at every offset mod 64 of the compact buffer -- in the request
    URI, the referer, and both."""
    c = _walk_cases()[name]
    p = _parser(oracle, c, options={lpa.OPT_FORCE_DIRECT: direct})
    r = decided_with(oracle, c, p)
    print("%s: %d lines, max wave events %d / %d, uri_overflow_waves %d" % (
        name, len(c.lines), max(c.wave_events(0)), max(c.wave_events(1)), r.diag["uri_overflow_waves"]))


# ---------------------------------------------------------- E: piece pass
@functools.lru_cache(None)
def _piece_cases():
    return uwc.piece_cases()


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("named", [False, True])
def test_piece_pass_gpu(oracle, named, direct):
    """E: wave piece totals 1..8, every ~37 up to ~700, and every multiple of
    64 and its neighbours; with the wildcard fields, and with one named
    parameter and a referer part only (most slots are skips, the referer
    stage has no query table)."""
    for c in _piece_cases():
        p = _parser(oracle, c, fields=uwc.NAMED_FIELDS if named else None, options={lpa.OPT_FORCE_DIRECT: direct})
        r = decided_with(oracle, c, p)
        assert r.counters["ok"] == len(c.lines)
        print("%s: piece totals %s, uri_overflow_waves %d" % (c.name, c.info["totals"], r.diag["uri_overflow_waves"]))


def test_piece_pass_device_table_gpu(oracle):
    """table.hip reads the slots the piece pass wrote: the device table equals
    the host table on query parameters, query strings and a referer part."""
    c = _piece_cases()[-1]
    p = lpa.HttpdLoglineParser("combined", lpa.get_possible_paths("combined"))
    r = p.parse_batch(c.data)
    assert r.counters["ok"] == len(c.lines) and r.diag["arena_ovf"] == 0, (r.counters, r.diag)
    _, res = r.copy_to_host()
    cols = [(f, str) for f in ("STRING:request.firstline.uri.query.k7", "STRING:request.firstline.uri.query.upper",
                               "STRING:request.referer.query.k7", "HTTP.QUERYSTRING:request.firstline.uri.query",
                               "HTTP.QUERYSTRING:request.referer.query", "HTTP.PATH:request.referer.path")]
    assert _device_vs_host_table(r, res, cols) == []


# ------------------------------------------------------- F: wave activity
def test_wave_activity_gpu(oracle):
    """F: batches of 1, 63, 64, 65, 127, 128, 129 lines, every third BAD in
    phase 1 (inactive lanes, and lanes whose line never reaches phase 2)."""
    for c in uwc.activity_cases():
        r = decided(oracle, c)
        assert r.counters["bad"] == len(c.bad)


# ------------------------------------------------------ G: several formats
def test_several_formats_gpu(oracle):
    """G: lanes of three LogFormats with different URI-stage counts share the
    walk rounds and the piece blocks (the SLOT instance), against the
    stateful oracle in order."""
    from test_emu_parity import mixed_lines
    c = uwc.mixed_case(mixed_lines(1024, 62))
    r = decided(oracle, c, options={lpa.OPT_ONE_PASS: 1})
    assert r.counters["ok"] > 900


# ------------------------------------------------------- H: a reused handle
def test_reused_handle_gpu(oracle):
    """H: a batch with large regions and many slots, then a different batch on
    the same handle: stale arena contents are never read."""
    big, small = _piece_cases()[-1], _walk_cases()["D3-req"]
    p = _parser(oracle, big)
    decided_with(oracle, big, p)
    decided_with(oracle, small, p)
    decided_with(oracle, big, p)
