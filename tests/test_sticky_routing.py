"""Sticky multi-format routing on overlapping formats, CPU part
(sticky_corpus.py: four Apache formats whose match sets overlap, so that the
routed format depends on the routing state and shows in the record).

The expectation is sticky_corpus.fold(), a left fold written from the Java
rule.  Here it is pinned from three sides: the corpus' construction against
four single-format oracles, the fold against the stateful oracle on every
sequence the GPU tests walk, and the CPU emulation of the device per-line code
against the fold, line by line.  The emulation routes one line at a time, so
the scan itself (the transition tables, their composition, the lane / chunk
tree of kernels.hip) is checked by tests/emu/route_emu.cpp, a stand-alone
program run under ASan + UBSan.  The GPU part is test_sticky_routing_gpu.py.
"""
import os
import subprocess

import pytest

import sticky_corpus as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "route_emu.cpp")
CORE_HDRS = [os.path.join(ROOT, "logparser_amd", "csrc", h) for h in ("lp_device.h", "lp_program.h")]
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
EMU_OK, EMU_BAD, EMU_FALLBACK = 0, 1, 2

SEQUENCES = sc.sequences()


@pytest.fixture(scope="module")
def records(oracle):
    return sc.Records(oracle)


@pytest.fixture(scope="module")
def fields(oracle):
    return oracle.possible_paths(sc.LOGFORMAT)


def _flat(name):
    kinds = [k for batch in SEQUENCES[name] for k in batch]
    return kinds, sc.fold(kinds)


def test_construction(oracle, records):
    """every kind's line matches exactly the formats of its match set (a V kind: the same tail
    with a plain URI; as written, the formats of its match set are undecided and the others BAD),
    and the overlapping kinds give different records in the formats they match"""
    for kind in list(sc.KINDS) + sc.V_KINDS:
        for i in (0, 5, 4095, 70000):
            line = sc.make_line(kind, i, ascii_uri=True)
            got = {f for f in range(sc.NF) if records.status(f, line) == oracle.OK}
            assert got == sc.match_set(kind), (kind, line)
            bad = {f for f in range(sc.NF) if records.status(f, line) == oracle.BAD}
            assert bad == set(range(sc.NF)) - got, (kind, line)
            if kind.startswith("V"):
                line = sc.make_line(kind, i)
                assert b"\xc3\xa9" in line
                st = [records.status(f, line) for f in range(sc.NF)]
                assert {f for f in range(sc.NF) if st[f] == oracle.UNSUPPORTED} == sc.match_set(kind), (kind, st)
                assert {f for f in range(sc.NF) if st[f] == oracle.BAD} == set(range(sc.NF)) - sc.match_set(kind)
    for i in (0, 5, 4095):
        a = sc.make_line("A", i)
        r0, r1 = records.record(0, a), records.record(1, a)
        assert r0["STRING:request.status.last"] == ["200"] and r0["BYTES:response.body.bytes"] == [str(sc.number(i))]
        assert r1["STRING:request.status.last"] == [str(sc.number(i))] and r1["BYTES:response.body.bytes"] == ["200"]
        b = sc.make_line("B", i)
        assert records.record(2, b) != records.record(3, b)
    # distinct lines: the client IP and the URI follow the index
    lines = sc.make_lines(["A"] * 70000)
    assert len(set(lines)) == len(lines)
    assert b"\xff" in sc.make_line("U", 3) and len(sc.make_line("A", 3, pad=300)) > 300


def test_fold_rule():
    """the fold on hand-written cases: the Java rule, and the unknown state's contract"""
    def states(kinds, state=0):
        return [r.state for r in sc.fold(kinds, state)]
    assert states(["A", "X1", "A", "B", "A", "N", "X3", "B", "A"]) == [0, 1, 1, 2, 0, 0, 3, 3, 0]
    assert states(["A", "B"], 3) == [0, 2] and states(["B", "A"], 1) == [2, 0]
    rows = sc.fold(["X1", "U", "A", "N", "B", "VA", "X2", "B", "N", "VB", "A"])
    assert [r.state for r in rows] == [1, None, None, None, None, None, 2, 2, 2, 2, 0]
    assert [r.cls for r in rows] == [sc.OK, sc.FALLBACK, sc.FALLBACK, sc.BAD_OR_FALLBACK, sc.FALLBACK, sc.FALLBACK,
                                     sc.OK, sc.OK, sc.BAD, sc.FALLBACK, sc.OK]
    assert [r.fmt for r in rows] == [1, None, None, None, None, None, 2, 2, None, None, 0]
    assert sc.fmt_ids(rows) == [1, 15, 15, 15, 15, 15, 2, 2, 2, 2, 0]


def test_sequences_shape():
    """what the sequences are for is in them: the placed lines at the scan's edges, whole lanes and
    chunks of overlapping lines, every (state, match set) pair, and few undecided lines"""
    for name, batches in SEQUENCES.items():
        kinds, rows = _flat(name)
        assert len(kinds) <= 8500 and sc.undecided_share(rows) <= 0.10, name
    kinds, rows = _flat("edge-last")
    for e in sc.EDGES:
        assert kinds[e - 1] in sc.EXCLUSIVE and rows[e - 1].state != rows[e - 2].state
        assert all(k in ("A", "B") for k in kinds[e:e + 63]) and rows[e + 62].state == rows[e - 1].state
    kinds, rows = _flat("edge-both")
    for e in sc.EDGES:
        assert kinds[e - 1] in sc.EXCLUSIVE and kinds[e] in sc.EXCLUSIVE and rows[e].state != rows[e - 1].state
    kinds, rows = _flat("edge-N")
    for e in sc.EDGES:
        assert match_empty(kinds[e - 1]) and match_empty(kinds[e]) and rows[e + 1].state == rows[e - 2].state != 0
    kinds, rows = _flat("lane-of-A")
    assert kinds[63] == "X1" and kinds[64:128] == ["A"] * 64 and kinds[128] == "X3"
    for name, fill, st in (("chunk-of-A", {"A"}, 1), ("chunk-of-B", {"B"}, 3), ("chunk-of-AB", {"A", "B"}, None)):
        kinds, rows = _flat(name)
        assert kinds[sc.CHUNK - 1] in sc.EXCLUSIVE and set(kinds[sc.CHUNK:2 * sc.CHUNK]) == fill
        assert st is None or (rows[sc.CHUNK - 1].state == st and rows[2 * sc.CHUNK].state == st)
    kinds, rows = _flat("transitions")
    assert kinds[:13] == sc.CYCLE and kinds[13:26] == sc.CYCLE and len(kinds) == 4200
    kinds, rows = _flat("transitions-all")
    lanes = {}  # (state before, match set) -> the lanes it occurs in
    for i in range(1, len(kinds)):
        lanes.setdefault((rows[i - 1].state, frozenset(sc.match_set(kinds[i]))), set()).add(i // sc.LANE)
    sets = [frozenset(s) for s in ({0}, {1}, {2}, {3}, {0, 1}, {2, 3}, set())]
    assert set(lanes) == {(s, m) for s in range(sc.NF) for m in sets}
    assert min(len(v) for v in lanes.values()) >= 20, {k: len(v) for k, v in lanes.items()}
    for n in sc.COUNTS:
        first, batch = SEQUENCES["count-%d" % n]
        assert first == ["X1"] and len(batch) == n and batch[-1] == "A" and (n == 1 or batch[0] == "X3")
    for at in sc.U_AT:
        kinds, rows = _flat("unknown-U-%d" % at)
        assert kinds[at] == "U" and all(r.state is None for r in rows[at:at + 71])
        assert all(r.state is not None for r in rows[at + 71:]) and all(r.state is not None for r in rows[:at])
        nxt = (at // sc.LANE + 1) * sc.LANE
        assert at + 70 > nxt + 1  # the undecided run crosses the next lane edge (from 4095: the chunk edge)
        kinds, rows = _flat("unknown-V-%d" % at)
        assert kinds[at] in sc.V_KINDS and all(r.state is not None for r in rows)
    kinds, rows = _flat("random")
    assert 30 < kinds.count("U") < 100 and 80 < sum(k in sc.V_KINDS for k in kinds) < 170
    assert sum(len(b) == 0 for b in SEQUENCES["empty-batch"]) == 1
    for end in ("A", "N", "U", "X2"):
        a, b = SEQUENCES["split-after-%s" % end]
        assert a[-1] == end and b[0] == "A"
    # ... and where the next batch's results depend on the state the handle carries: they differ
    # from those of a handle that starts the batch at format 0
    carried = ["split-after-A", "split-after-N", "split-after-U", "empty-batch", "queue-all"]
    carried += ["carry-%d" % n for n in (1, 64, 4096, 4097)] + ["count-1"]
    for name in carried:
        batches = SEQUENCES[name]
        rows, first = _flat(name)[1], len(batches[0])
        for b in batches[1:]:
            assert sc.fold(b, 0) != rows[first:first + len(b)] or not b, name
            first += len(b)


def match_empty(kind):
    return kind != "U" and not sc.match_set(kind)


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_fold_against_stateful_oracle(oracle, records, fields, name):
    """the stateful oracle (one parser, the four formats) walks the sequence: on every line the
    fold decides, its status and record are the fold's (the record: the single-format oracle of the
    routed format, with that format's own possible paths)"""
    kinds, rows = _flat(name)
    o = oracle.Oracle(sc.LOGFORMAT, fields)
    for i, (k, row) in enumerate(zip(kinds, rows)):
        line = sc.make_line(k, i)
        st, js = o.parse_raw(line)
        if row.cls == sc.OK:
            assert st == oracle.OK, (i, k, st)
            assert sc.same_record(js, records.record_json(row.fmt, line)), (i, k, row)
        elif row.cls == sc.BAD:
            assert st == oracle.BAD, (i, k, st)


# the emulation routes one line at a time: where a line sits in a lane, chunk or batch is nothing
# to it, so it walks the sequences that differ in what follows what, not those that differ in where
EMU_SEQUENCES = ["transitions", "transitions-all", "random", "lane-of-A", "queue-all", "queue-none", "count-65",
                 "unknown-U-63", "unknown-V-63", "unknown-U-4096", "unknown-V-4096", "split-after-U", "split-after-N"]


@pytest.mark.parametrize("name", EMU_SEQUENCES)
def test_emulation_against_fold(emu, records, fields, name):
    """the device per-line code on the CPU (both scanner modes), one parser walking the sequence:
    exact on every line the fold decides, FALLBACK on every line that must be, and on no other
    line but the failing lines of an unknown state"""
    kinds, rows = _flat(name)
    e = emu.Emu(sc.LOGFORMAT, fields)
    assert e.status == 0, e.err
    for i, (k, row) in enumerate(zip(kinds, rows)):
        line = sc.make_line(k, i)
        st, js = e.parse_raw(line)
        if row.cls == sc.OK:
            assert st == EMU_OK, (i, k, st)
            assert sc.same_record(js, records.record_json(row.fmt, line)), (i, k, row)
        elif row.cls == sc.BAD:
            assert st == EMU_BAD, (i, k, st)
        elif row.cls == sc.FALLBACK:
            assert st == EMU_FALLBACK, (i, k, st)
        else:
            assert st in (EMU_BAD, EMU_FALLBACK), (i, k, st)


def _build(target, flags):
    os.makedirs(BUILD, exist_ok=True)
    newest = max(os.path.getmtime(p) for p in [EMU_SRC] + CORE_HDRS)
    if os.path.exists(target) and os.path.getmtime(target) >= newest:
        return target
    tmp = "%s.%d.tmp" % (target, os.getpid())  # renamed into place: parallel workers never see half a file
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-o", tmp] + flags + [EMU_SRC], check=True)
    os.replace(tmp, target)
    return target


def test_scan_algebra_sanitized_program():
    """fmt_table / fmt_compose / fmt_apply (csrc/lp_device.h) against a plain loop of the Java rule
    for every format count, match word and state; the identity, composition against application,
    associativity; and the scan's lane / chunk tree against the serial fold -- under ASan + UBSan,
    a program with its own main, run directly"""
    prog = _build(os.path.join(BUILD, "route_emu_san"), ASAN)
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "8388608 table entries" in r.stdout and " 0 differ" in r.stdout, r.stdout
