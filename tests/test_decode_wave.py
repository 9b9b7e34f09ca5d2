"""Corpora of the URI kernels' dense decode pass (decode_wave_corpus), CPU
part: every line of every case through the emulation of the device per-line
code (the serial query_piece, which runs the same name and value parts)
against the oracle, none FALLBACK; and the corpora's own claims -- the planted
counts of pieces whose value needs decoding, per wave and per 64-piece block,
are what count_pv re-derives from the URIs.  The GPU part is
test_decode_wave_gpu.py."""
import decode_wave_corpus as dwc
import uri_wave_corpus as uwc
from test_emu_parity import mixed_lines
from test_uri_wave import check

PW, CAPD = dwc.PW, dwc.CAPD


def test_cases_decided(oracle, emu):
    for c in dwc.all_cases():
        assert len(c.lines) % PW == 0 and not c.bad and not c.defective
        assert max(len(l) for l in c.lines) < 8191
        assert check(oracle, emu, c) == len(c.lines), c.name
    named = dwc.count_cases()
    assert check(oracle, emu, named, fields=dwc.NAMED_FIELDS) == len(named.lines)


def test_mixed_formats_decided(oracle, emu):
    c = dwc.mixed_decode_case(mixed_lines(512, 62))
    assert check(oracle, emu, c) > 450
    assert sum(dwc.count_pv(m.group(2).decode()) for m in map(uwc._REQ.search, c.lines) if m) > 500


def test_planted_counts():
    assert CAPD >= PW  # an empty buffer takes any block
    for c in dwc.all_cases():
        got = dwc.wave_block_pv(c)
        assert got == c.info["pv"], c.name
        # per wave: the blocks' sum is the lines' count_pv, and the pieces are uri_wave_corpus's
        for w, blocks in enumerate(got):
            uris = [u for k in range(PW * w, PW * w + PW) for u in c.uris[k] if u is not None]
            assert sum(blocks) == sum(dwc.count_pv(u) for u in uris), (c.name, w)
            assert len(blocks) == (sum(uwc.count_pieces(u) for u in uris) + PW - 1) // PW, (c.name, w)
        assert [sum(uwc.count_pieces(u) for u in us if u) for us in c.uris] == \
               [sum(len(dwc.piece_flags(u)) for u in us if u) for us in c.uris]
    by = {c.name: c for c in dwc.all_cases()}
    # N: the first n pieces of one round; the last wave: 64 arriving when 1 waits
    n = by["N-counts"]
    assert {0, 1, 2, 63, 64, 65, CAPD - 1, CAPD, CAPD + 1, 128, 255, 256} == set(dwc.COUNTS)
    assert [sum(b) for b in n.info["pv"][:-1]] == dwc.COUNTS and all(len(b) == 4 for b in n.info["pv"])
    assert n.info["pv"][-1] == [1, 64, 0, 0]
    assert n.wave_pieces() == [dwc.ROUND] * len(n.info["pv"])
    # P
    p = by["P-placement"].info["pv"]
    assert p[0][1:] == [0, 0, 0] and p[0][0] > 0 and p[1][:3] == [0, 0, 0] and p[1][3] > 0
    assert p[2] == [1, 1, 1, 1]
    assert sum(p[3]) == 60 and max(uwc.count_pieces(u[0]) for u in by["P-placement"].uris[3 * PW:4 * PW] if u[0]) == 300
    assert p[4] == p[5] == p[6] == [32] * 4
    assert p[7] == [0, 0, 0, 6, 6] and p[8][3:5] == [64, 64] and p[8][8] == 1
    stages = lambda w: {(bool(dwc.count_pv(u[0] or "")), bool(dwc.count_pv(u[1] or "")))
                        for u in by["P-placement"].uris[PW * w:PW * w + PW]}
    assert stages(4) == {(True, False)} and stages(5) == {(False, True)} and stages(6) == {(True, True)}
    # V: every padding of the decoder's last word, the long values
    assert {len(v.replace("%7E", "~")) for v in dwc.VALUES if v.startswith("+x") or v == "+" or v.endswith("%7E")} >= set(range(1, 10))
    assert sum(map(sum, by["V-values"].info["pv"])) == 4 * len(dwc.VALUES)
    assert max(len(u[0]) for u in by["V-long2000"].uris) == 2005 and by["V-long2000"].uri_bytes() < 4096
    assert max(len(u[0]) for u in by["V-long6000"].uris) == 6104 and 8512 * 4 > by["V-long6000"].uri_bytes() > 8512 + 1024
    # M: rewritten names with decoded values, in the request URI and the referer
    assert any("n|m=a+b" in u[0] and u[1] and "Upper=%41" in u[1] for u in by["M-names"].uris)
