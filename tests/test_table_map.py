"""lp_result_table_map, CPU part: the Arrow-to-dict helper, the derivation of
the expected maps from the oracle's records (table_map_ref), and that the GPU
corpora plant what test_table_map_gpu.py relies on."""
import numpy as np

import logparser_amd as lpa
import table_map_ref as tmr
import uri_wave_corpus as uwc

REQ = "STRING:request.firstline.uri.query.*"
REF = "STRING:request.referer.query.*"
HEAD = '1.2.3.4 - - [10/Oct/2026:13:55:36 +0200] "GET %s HTTP/1.1" 200 5 "%s" "ua"'


def _arrow(rows):
    """hand-built Arrow arrays of rows: a list of (key, value) pairs, or None"""
    valid, eo, ko, vo, kc, vc = [], [0], [0], [0], b"", b""
    for r in rows:
        valid.append(0 if r is None else 1)
        for k, v in r or ():
            kc += k.encode()
            vc += v.encode()
            ko.append(len(kc))
            vo.append(len(vc))
        eo.append(len(ko) - 1)
    i64 = lambda a: np.array(a, dtype=np.int64)
    return (np.array(valid, dtype=np.uint8), i64(eo), i64(ko), np.frombuffer(kc, dtype=np.uint8), i64(vo),
            np.frombuffer(vc, dtype=np.uint8))


def test_maps_from_arrow():
    """an empty map, an invalid row, a "" key, an empty value, UTF-8, and the
    entry order kept"""
    rows = [[("b", ""), ("a", "3"), ("", "x"), ("c", "A")], [], None, [("", "")], [("é", "ü"), ("k", "v")], None]
    got = lpa.maps_from_arrow(*_arrow(rows))
    assert got == [None if r is None else dict(r) for r in rows]
    assert got[1] == {} and got[2] is None and got[3] == {"": ""}
    assert list(got[0].items()) == rows[0] and list(got[4]) == ["é", "k"]
    assert lpa.maps_from_arrow(*_arrow([])) == []
    # torch-free: any sequence of ints and bytes works
    v, eo, ko, kc, vo, vc = _arrow(rows)
    assert lpa.maps_from_arrow(list(v), list(eo), list(ko), kc.tobytes(), list(vo), vc.tobytes()) == got


def test_derivation_on_handwritten_lines(oracle):
    """The oracle's record keeps every value of a repeated name, in order,
    under one key (not one value per name): the rule "the last non-null value
    wins" is applied here, by expected_map."""
    fields = [REQ, REF]
    o = oracle.Oracle("combined", fields)
    st, rec = o.parse(HEAD % ("/p?a=1&A=2&b&a=3&=x&&c=%41", "http://h/r?Z=1&z=&y"))
    assert st == oracle.OK
    assert rec["STRING:request.firstline.uri.query.a"] == ["1", "2", "3"]  # all three deliveries, lower-cased name
    assert rec["STRING:request.firstline.uri.query"] == ["x"]              # the empty name: the prefix itself
    assert tmr.expected_map(rec, REQ) == {"a": "3", "b": "", "": "x", "c": "A"}
    assert tmr.expected_map(rec, REF) == {"z": "", "y": ""}
    assert tmr.deliveries(rec, REQ) == 6 and tmr.deliveries(rec, REF) == 3
    # no query at all, and a referer "-": empty maps (the record exists)
    st, rec = o.parse(HEAD % ("/p", "-"))
    assert st == oracle.OK and tmr.expected_map(rec, REQ) == {} and tmr.expected_map(rec, REF) == {}
    # nulls are ignored, longs are delivered as their decimal string
    fake = {"T:p.k": ["v", None], "T:p.n": [None], "T:p.l": [{"l": -7}], "T:px.k": ["no"], "U:p.k": ["no"], "T:p": ["e"]}
    assert tmr.expected_map(fake, "T:p.*") == {"k": "v", "l": "-7", "": "e"}


def test_gpu_corpora_plant_their_cases(oracle):
    """piece_cases() under the wildcard fields: a row of >= 300 pieces, rows
    without entries, repeated keys that collapse (through case folding too),
    every multiple of 64 among the per-wave piece totals."""
    cases = uwc.piece_cases()
    totals = set()
    most, empty, collapsed, folded = 0, 0, 0, 0
    for c in cases:
        totals.update(c.wave_pieces())
        ref = tmr.oracle_maps(oracle, c.name, "combined", [REQ, REF], c.lines, [REQ, REF])
        for k, m in enumerate(ref):
            assert m is not None, (c.name, k)
            n = m["#deliveries"][REQ] + m["#deliveries"][REF]
            assert n == sum(uwc.count_pieces(u) for u in c.uris[k] if u is not None), (c.name, k)
            most = max(most, n)
            empty += not m[REQ] and not m[REF]
            collapsed += m["#deliveries"][REQ] > len(m[REQ])
            uri = c.uris[k][0] or ""
            if "K7=" in uri and "k7=" in uri and "Upper=" in uri:
                assert "k7" in m[REQ] and "K7" not in m[REQ] and "upper" in m[REQ] and "Upper" not in m[REQ]
                folded += 1
    assert most >= 300 and empty > 0 and collapsed > 0 and folded > 0, (most, empty, collapsed, folded)
    assert all(t in totals for t in range(64, 705, 64)), sorted(totals)
