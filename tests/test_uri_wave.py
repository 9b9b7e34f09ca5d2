"""Boundary corpora of the URI kernels' wave-cooperative code
(uri_wave_corpus), CPU part: every family through the emulation of the device
per-line code, each line in place in its batch buffer, against the oracle.
The emulation runs the serial walk and piece pass (uri_walk_fast,
query_pieces_serial), so this validates the corpora themselves -- the oracle
decides every line, none is FALLBACK, the planted event / piece / block counts
are what a few lines of Python re-derive -- and pins the serial code on the
same edges.  The GPU part is test_uri_wave_gpu.py."""
import uri_wave_corpus as uwc
from test_emu_parity import COOKIE_FMT, MIXED, UPSTREAM_FMT, mixed_lines

FMTS = {"combined": "combined", "cookie": COOKIE_FMT, "upstream": UPSTREAM_FMT, "mixed": MIXED}
_FIELDS = {}

# B / C on the CPU: around where the kernel's compact buffer ends today (the
# GPU part locates that boundary itself; here any sizes serve)
B_TOTALS = (1024, 8496, 8512, 8528, 17024, 34048, 40000 // 16 * 16, 68096)
C_URI_TOTAL = 4224
C_TOKENS = tuple(range(16, 137, 8))


def fields_of(oracle, fmt):
    if fmt not in _FIELDS:
        _FIELDS[fmt] = oracle.possible_paths(FMTS[fmt])
    return _FIELDS[fmt]


def check(oracle, emu, case, fields=None):
    """every line of the case, parsed in place in its buffer by the emulation,
    equals the oracle (stateful: in order); neither is FALLBACK / UNSUPPORTED;
    the lines planted BAD are BAD.  Returns the number of OK lines."""
    fields = fields or fields_of(oracle, case.fmt)
    o = oracle.Oracle(FMTS[case.fmt], fields)
    e = emu.Emu(FMTS[case.fmt], fields)
    assert e.status == 0, e.err
    got = e.parse_batch_raw(case.data)
    assert len(got) == len(case.lines), case.name
    ok = 0
    for k, (l, g) in enumerate(zip(case.lines, got)):
        s1, r1 = o.parse_raw(l)
        assert s1 in (oracle.OK, oracle.BAD) and g[0] in (0, 1), (case.name, k, l, s1, g[0])
        assert s1 == g[0], (case.name, k, l, s1, g[0])
        assert r1 == g[1], (case.name, k, l, r1, g[1])
        if k not in case.defective and case.fmt != "mixed":  # (a repaired URI may be BAD in the reference)
            assert (s1 == oracle.BAD) == (k in case.bad), (case.name, k, l)
        ok += s1 == oracle.OK
    return ok


def test_gather_geometry(oracle, emu):
    c = uwc.gather_geometry()
    starts = {(s[0][0] % 16, s[0][1] % 16) for s in c.spans[:256]}
    assert len(starts) == 256
    assert {s[0][1] - s[0][0] for s in c.spans[256:]} == {1, 16, 17}
    assert any(s[0][0] % 16 == 0 and s[0][1] - s[0][0] == 16 for s in c.spans[256:])
    assert check(oracle, emu, c) == len(c.lines) == 304
    # the same lines in a buffer that starts at another address mod 16
    for base in (1, 15):
        c = uwc.gather_geometry(base)
        assert {((base + s[0][0]) % 16, (base + s[0][1]) % 16) for s in c.spans[:256]} == starts
        assert check(oracle, emu, c) == 304


def test_sparse_waves(oracle, emu):
    for c in uwc.sparse_waves():
        assert len(c.lines) == 64
        assert check(oracle, emu, c) == 64 - len(c.bad)
        assert (c.wave_blocks()[0] == 0) == (c.info["uri_lanes"] == 0)


def test_partial_last_block(oracle, emu):
    cases = uwc.partial_last_block()
    assert sorted(len(c.data) % 16 for c in cases) == list(range(16))
    for c in cases:
        assert not c.data.endswith(b"\n")
        assert check(oracle, emu, c) == 6


def test_path_tiers(oracle, emu):
    for T in B_TOTALS:
        c = uwc.wave_with_total(T)
        assert c.uri_bytes() == T and c.wave_blocks() == [T // 16]
        assert check(oracle, emu, c) == 64
    for v in ("long", "defect"):
        c = uwc.wave_with_total(8528, v)
        assert c.uri_bytes() == 8528 and len(c.defective) == (3 if v == "defect" else 0)
        assert max(len(l) for l in c.lines) < 8191
        assert check(oracle, emu, c) == 64


def test_list_and_pair_tokens(oracle, emu):
    for n in C_TOKENS:
        assert check(oracle, emu, uwc.cookie_wave(C_URI_TOTAL, n)) == 64
        assert check(oracle, emu, uwc.upstream_wave(C_URI_TOTAL, n)) == 64


def test_cooperative_walk(oracle, emu):
    cases = uwc.walk_cases()
    for c in cases:
        ok = check(oracle, emu, c)
        assert ok >= len(c.lines) - len(c.defective), c.name  # (a repaired URI may be BAD in the reference)
    by = {c.name: c for c in cases}
    # D1: every k of WALK_K starts at every position of a round (request stage)
    c = by["D1-req"]
    seen = set()
    for w in range(len(c.lines) // 64):
        e = 0
        for k in range(64 * w, 64 * w + 64):
            u = c.uris[k][0]
            n = uwc.count_events(u) if u else 0
            if k > 64 * w and n:
                seen.add((n, e % 64))
            e += n
    for n in uwc.WALK_K[1:]:
        assert {p for (m, p) in seen if m == n} == set(range(64)), n
    assert max(c.wave_blocks()) * 16 + 16 <= 8192  # (one compact buffer's worth: no tier change intended)
    # D2: the planted wave totals
    c = by["D2"]
    assert c.wave_events(0) == c.info["totals"] == [63, 64, 65, 127, 128, 129]
    # D3: every event of every placed URI at round positions 63 and 0
    for where in ("req", "ref", "both"):
        c = by["D3-" + where]
        want = {(u, j, r) for u, _ in uwc.PLACED for j in range(uwc.count_events(u)) for r in (63, 0)}
        got = set()
        for k, j, r in c.info["placed"]:
            st = 1 if where == "ref" else 0
            uri = c.uris[k][st][len(uwc.REF_HOST) if st else 0:]
            before = sum(uwc.count_events(c.uris[i][st] or "") for i in range(k // 64 * 64, k))
            assert (before + j) % 64 == r, (c.name, k, j, r)
            got.add((uri, j, r))
        assert got == want
        assert len(c.defective) == 2 * sum(uwc.count_events(u) for u, d in uwc.PLACED if d)
    # D4: the runs of '&' start at all 64 offsets mod 64 of the compact buffer
    assert uwc.amp_run_offsets(by["D4-req"]) == set(range(64))
    assert uwc.amp_run_offsets(by["D4-ref"]) == set(range(64))
    assert uwc.count_events(by["D4-req"].info["uri"]) == 132


def test_piece_pass(oracle, emu):
    assert set(range(1, 9)) <= set(uwc.PIECE_TOTALS) and max(uwc.PIECE_TOTALS) >= 700
    for m in range(64, 705, 64):
        assert {m - 1, m, m + 1} <= set(uwc.PIECE_TOTALS)
    assert max(uwc.piece_counts(700)) == 300 and max(uwc.piece_counts(129)) > 64
    named = None
    for c in uwc.piece_cases():
        assert c.wave_pieces() == c.info["totals"], c.name
        assert max(len(l) for l in c.lines) < 8191
        assert check(oracle, emu, c) == len(c.lines)
        named = c
    # only one named parameter and a referer part: most pieces are skipped
    assert check(oracle, emu, named, fields=uwc.NAMED_FIELDS) == len(named.lines)


def test_wave_activity(oracle, emu):
    for c in uwc.activity_cases():
        assert len(c.bad) == len(c.lines) // 3
        assert check(oracle, emu, c) == len(c.lines) - len(c.bad)


def test_several_formats(oracle, emu):
    c = uwc.mixed_case(mixed_lines(1024, 62))
    assert check(oracle, emu, c) > 900
