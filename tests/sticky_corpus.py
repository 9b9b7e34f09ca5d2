"""Sticky multi-format routing: a constructed corpus of overlapping formats.

Four Apache LogFormats in one handle whose match sets overlap, so that the
format a line is routed to depends on the routing state (the active format of
HttpdLogFormatDissector.dissect) and shows in the record:

    F0 = pre + '%>s %b'        F2 = pre + '%>s %b %D'
    F1 = pre + '%b %>s'        F3 = pre + '%b %>s %D'

%>s is a no-space string, %b is [0-9]+|- and %D is digits, so a line's tail
fixes the set of formats that match it (KINDS).  On an `A` line (tail "200 n")
F0 gives status 200 and bytes n, F1 bytes 200 and status n.

Two more kinds are undecided on the device: `U` (a 0xFF byte in the user
field: every undecided bit of the match word, the routing state becomes
unknown) and `V<kind>` (U+00E9 in the request URI: the line is FALLBACK, its
routing is decided by its tail).

The expectation is fold(): a left fold written from the Java rule (the active
format first, else the first format that matches, else the state stays) plus
the contract of the unknown state (csrc/lp_device.h: from an undecided state a
line is decided only when every state leads to the same format).  It knows
nothing of transition tables, lanes, chunks or batches.  The records come from
four single-format oracles.

sequences() places the kinds at the edges of the routing scan (64 lines per
lane, 4096 lines per chunk); a sequence is a list of batches of one handle,
folded as one concatenation.  Shared by test_sticky_routing.py (oracle, CPU
emulation) and test_sticky_routing_gpu.py.
"""
import json
import random
from collections import namedtuple

PRE = '%h %l %u %t "%r" '
FORMATS = [PRE + "%>s %b", PRE + "%b %>s", PRE + "%>s %b %D", PRE + "%b %>s %D"]
LOGFORMAT = "\n".join(FORMATS)
NF = len(FORMATS)
FMT_UNKNOWN = 15  # csrc/lp_program.h
LANE, CHUNK = 64, 4096  # lines per lane and per wave of the routing scan

# kind -> (tail, the formats that match)
KINDS = {
    "X0": ("w200 {n}", {0}),
    "X1": ("{n} w404", {1}),
    "X2": ("w200 {n} 77", {2}),
    "X3": ("{n} w404 77", {3}),
    "A": ("200 {n}", {0, 1}),
    "B": ("200 {n} 77", {2, 3}),
    "N": ("w{n}", set()),
    "N2": ("w w {n} w", set()),
}
EXCLUSIVE = ("X0", "X1", "X2", "X3")
V_KINDS = ["V" + k for k in ("X0", "X1", "X2", "X3", "A", "B")]
METHODS = ["GET", "GET", "GET", "POST", "GET", "HEAD", "GET", "PROPFIND", "GET", "GET", "DELETE"]


def base_kind(kind):
    return kind[1:] if kind.startswith("V") else kind


def match_set(kind):
    """the formats whose regex matches a line of this kind (U: not decided)"""
    return KINDS[base_kind(kind)][1]


def number(i):
    """the per-line number n: three digits (a status code when it is routed to %>s), never 200"""
    n = 100 + (i * 37) % 900
    return 201 if n == 200 else n


def make_line(kind, i, pad=0, query=False, ascii_uri=False):
    """line i of a sequence: client IP, URI and n derived from i; pad: the length %u is padded to;
    query: a query string on the request; ascii_uri: a V kind's tail with a plain URI"""
    user = b"-"
    if kind == "U":
        user, kind = b"u\xffx", "A"
    if pad:
        user = user + b"p" * (pad - len(user))
    uri = b"/p/%d" % i
    if kind.startswith("V") and not ascii_uri:
        uri += b"/caf\xc3\xa9"
    if query:
        uri += b"?a=%d&b=x%%41y+z&c=%d" % (i, i * 7)
    tail = KINDS[base_kind(kind)][0].format(n=number(i)).encode()
    return b'10.%d.%d.%d - %s [01/Jan/2021:00:00:%02d +0000] "%s %s HTTP/1.1" %s' % (
        (i >> 16) & 255, (i >> 8) & 255, i & 255, user, i % 60, METHODS[i % len(METHODS)].encode(), uri, tail)


def make_lines(kinds, first=0, **kw):
    return [make_line(k, first + j, **kw) for j, k in enumerate(kinds)]


# ---------------------------------------------------------------- the reference
OK, BAD, FALLBACK, BAD_OR_FALLBACK = "ok", "bad", "fallback", "bad-or-fallback"
Row = namedtuple("Row", "cls fmt state")  # fmt: the format of an OK line; state: after the line, None = unknown


def step(s, m):
    """HttpdLogFormatDissector.dissect: the active format when it matches, else the first that does"""
    return s if (s in m or not m) else min(m)


def fold(kinds, state=0):
    """[Row] of a sequence of kinds from the handle's state (0 for a new handle)"""
    out = []
    s = state
    for k in kinds:
        if k == "U":
            s = None
            out.append(Row(FALLBACK, None, s))
            continue
        m = match_set(k)
        if s is None:
            ends = {step(x, m) for x in range(NF)}
            s2 = ends.pop() if len(ends) == 1 else None
        else:
            s2 = step(s, m)
        if not m:
            cls = BAD if s is not None else BAD_OR_FALLBACK
        elif s2 is None:
            cls = FALLBACK
        else:
            cls = FALLBACK if k.startswith("V") else OK
        out.append(Row(cls, s2 if cls == OK else None, s2))
        s = s2
    return out


def undecided_share(rows):
    """the lines no record is compared on: must-be-FALLBACK and BAD-or-FALLBACK"""
    return sum(1 for r in rows if r.cls in (FALLBACK, BAD_OR_FALLBACK)) / max(1, len(rows))


def fmt_ids(rows):
    return [FMT_UNKNOWN if r.state is None else r.state for r in rows]


class Records:
    """the expected records: one single-format oracle per format, each with that format's own
    possible paths"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.parsers = [oracle.Oracle(f, oracle.possible_paths(f)) for f in FORMATS]

    def status(self, f, line):
        return self.parsers[f].parse_raw(line)[0]

    def record_json(self, f, line):
        st, js = self.parsers[f].parse_raw(line)
        assert st == self.oracle.OK, (f, line, st)
        return js

    def record(self, f, line):
        return json.loads(self.record_json(f, line))


def same_record(a, b):
    """two records' JSON texts, compared as parsed JSON (equal texts need no parsing)"""
    return a == b or json.loads(a) == json.loads(b)


# ---------------------------------------------------------------- the sequences
def keeping(n, placed, state=0):
    """n kinds: `placed` {index: kind}, every other line the overlapping kind that keeps the state
    the fold has there (A in state 0 / 1, B in state 2 / 3; A while it is unknown), so that every
    record depends on the last placed line before it"""
    out = []
    s = state
    for i in range(n):
        k = placed.get(i) or ("B" if s in (2, 3) else "A")
        out.append(k)
        s = fold([k], s)[0].state
    return out


CYCLE = "X0 A B X1 A B X2 B A X3 B A N".split()
EDGES = (LANE, CHUNK, 2 * CHUNK)
COUNTS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
U_AT = (63, 64, 4095, 4096)
N_TRANSITIONS = 4200


def transitions():
    return [CYCLE[i % len(CYCLE)] for i in range(N_TRANSITIONS)]


def all_transitions():
    """CYCLE starts from the same state every time round, so it walks 13 of the 28 (state, match
    set) pairs; this one sets each state with its exclusive line and follows it with each kind in
    turn: all 28, in a period of 56 lines that moves through the lanes"""
    period = [k for s in EXCLUSIVE for nxt in EXCLUSIVE + ("A", "B", "N") for k in (s, nxt)]
    return [period[i % len(period)] for i in range(N_TRANSITIONS)]


def _edge_sequences():
    n = 2 * CHUNK + 208
    seqs = {}
    # the state last changed by the line before an edge; by that line and the edge's line; and
    # kept by a failing line on either side of the edge
    seqs["edge-last"] = keeping(n, {0: "X3", 63: "X1", 4095: "X3", 8191: "X1"})
    seqs["edge-both"] = keeping(n, {0: "X2", 63: "X3", 64: "X1", 4095: "X2", 4096: "X3", 8191: "X1", 8192: "X2"})
    seqs["edge-first"] = keeping(n, {0: "X1", 64: "X3", 4096: "X1", 8192: "X3"})
    seqs["edge-N"] = keeping(n, {0: "X2", 62: "X1", 63: "N", 64: "N2", 4094: "X3", 4095: "N2", 4096: "N",
                                 8190: "X1", 8191: "N", 8192: "N"})
    # a lane of 64 A lines exactly; chunk 1 of 4096 overlapping lines exactly (A after X1, B after
    # X3): set by the last line of chunk 0, read by the first line of chunk 2
    seqs["lane-of-A"] = keeping(400, {0: "X3", 63: "X1", 128: "X3", 191: "X1", 256: "X2"})
    seqs["chunk-of-A"] = keeping(n, {0: "X3", 4095: "X1"})
    seqs["chunk-of-B"] = keeping(n, {4095: "X3"})
    mixed = keeping(n, {0: "X3", 4095: "X1"})
    for i in range(CHUNK, 2 * CHUNK):  # chunk 1 of A and B lines mixed, ending on a run of B
        mixed[i] = "A" if (i * 7 // 5) % 3 and i < 2 * CHUNK - 70 else "B"
    seqs["chunk-of-AB"] = mixed
    return seqs


def _unknown_sequence(at, kind):
    """`kind` (U or a V kind) at index `at`; then 70 overlapping and failing lines across the next
    lane edge (and, from 4095 / 4096, inside the next chunk), an exclusive line, and decided lines"""
    n = max(at + 400, 1000)
    placed = {0: "X1", at: kind, at + 71: "X3", at + 200: "X1"}
    run = "A B N A A B N2 B".split()
    for j in range(70):
        placed[at + 1 + j] = run[j % len(run)]
    return keeping(n, placed)


def random_kinds(n=6000, seed=20261021):
    rng = random.Random(seed)
    plain = ["X0", "X1", "X2", "X3", "A", "A", "A", "B", "B", "B", "N", "N2"]
    out = []
    for _ in range(n):
        x = rng.random()
        out.append("U" if x < 0.01 else rng.choice(V_KINDS) if x < 0.03 else rng.choice(plain))
    return out


def split_at(kinds, *cuts):
    cuts = (0,) + cuts + (len(kinds),)
    return [kinds[a:b] for a, b in zip(cuts, cuts[1:])]


def sequences():
    """{name: [batch of kinds, ...]}: every sequence the CPU and the GPU tests walk; the batches
    of a sequence go through one handle in order (the line index runs on across them)"""
    out = {}
    for name, s in _edge_sequences().items():
        out[name] = [s]
    out["transitions"] = [transitions()]
    out["transitions-all"] = [all_transitions()]
    for n in COUNTS:  # a batch that leaves state 1, then n lines: X3 ... A (one line: the A)
        out["count-%d" % n] = [["X1"], keeping(n, {0: "X3", n - 1: "A"}) if n > 1 else ["A"]]
    for at in U_AT:
        out["unknown-U-%d" % at] = [_unknown_sequence(at, "U")]
        out["unknown-V-%d" % at] = [_unknown_sequence(at, "VA" if at % 2 else "VB")]
    out["queue-all"] = [["X1"], ["A"] * 4200]
    out["queue-none"] = [[("X0", "X1", "N", "X2", "X3", "N2")[i % 6] for i in range(4200)]]
    out["random"] = [random_kinds()]
    t = transitions()
    for cut in (1, 64, 4096, 4097):
        out["split-%d" % cut] = split_at(t, cut)
    # a batch that ends on `end`, the next begins with A: after "X1 A", where the state is 1 (an A
    # line tells 0 from 1 only; after X2 it reads 0 whatever was carried)
    for end in ("A", "N", "U", "X2"):
        s = transitions()
        cut = 2085
        assert s[cut - 2:cut + 1] == ["X1", "A", "B"]
        s[cut - 1], s[cut] = end, "A"
        out["split-after-%s" % end] = split_at(s, cut)
    assert t[2005:2007] == ["X1", "A"]
    out["empty-batch"] = split_at(t, 2006, 2006)
    # CYCLE's state is 0 at 1, 64, 4096 and 4097, the state of a new handle: batches of those sizes
    # that leave state 3 to lines that keep it
    for n in (1, 64, 4096, 4097):
        out["carry-%d" % n] = [keeping(n, {n - 1: "X3"}), keeping(200, {100: "X1"}, state=3), keeping(70, {}, state=1)]
    return out
