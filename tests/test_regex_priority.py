"""The LogFormat matcher against an independent regex engine, CPU part.

match_line and its candidate enumerators (csrc/lp_device.h) claim java.util.regex's leftmost-first priority,
exactly, through hand-derived shortcuts: the `det` marking, the need / kth_from_end pruning of greedy `.*`, the
literal-aware first candidates, cand_next per kind, the inlined short literal against the long-literal path, the
quote-count / line-tail prefilters and the first-leaf match.  Every other test compares that code with oracle/,
whose jregex.c is this project's own reading of the same semantics.  Here the oracle and the CPU emulation of the
device code are each compared with Python's `re` (regex_ref.py) line by line, on corpora in which the formats' own
separators occur inside the field values (regex_corpus.py).  The GPU part is test_regex_priority_gpu.py.
"""
import collections
import json
import re
import time

import pytest

import regex_corpus as rc
import regex_ref as rr

EMU_OK, EMU_BAD, EMU_FALLBACK = 0, 1, 2


def test_java_to_py():
    """the translation: \\Q..\\E is literal text, '.' and '$' are Java's, and whatever it does not know raises"""
    assert re.compile(rr.java_to_py(r"^\Q.*[\E(a+?)\Q$\E$"), re.ASCII).search(".*[aaa$").group(1) == "aaa"
    dot = re.compile(rr.java_to_py("^a.b$"), re.ASCII)
    assert dot.search("a b") and not dot.search("a\rb") and not dot.search("a\nb") and not dot.search("a\x85b")
    end = re.compile(rr.java_to_py("^a$"), re.ASCII)
    assert end.search("a") and end.search("a\n") and end.search("a\r\n") and end.search("a\r") and not end.search("a\n\n")
    sp = re.compile(rr.java_to_py(r"^[^\s]*$"), re.ASCII)
    assert all(not sp.search("a%sb" % c) for c in " \t\n\x0b\x0c\r") and sp.search("a\x1cb") and sp.search("a\xa0b")
    for bad in (r"a*+", r"a++", r"a?+", r"a{2}+", r"a{2", r"\p{L}", r"\h", r"\d", r"\w", r"\b", r"\1", r"(?i)a", r"(?=a)",
                r"(?<n>a)", r"(?>a)", r"[a&&b]", r"[a[b]]", r"[\d]", r"a**", r"a*?+", r"*a", r"\Qa", "a\tb", r"\R", r"\z"):
        with pytest.raises(rr.Untranslatable):
            rr.java_to_py(bad)


@pytest.mark.parametrize("name", list(rr.FORMATS))
def test_regex_translates(oracle, emu, name):
    """the printed regex translates and compiles; one group per requested path, each a path of the format; the
    corpus knows every token's regex; and the format is on the device (a format that is not would have to leave
    this list, with its reason: emu.status)"""
    ref = rr.Ref(oracle, name)
    assert ref.re.groups == len(ref.groups) == len(set(ref.groups))
    assert set(ref.groups) <= set(oracle.possible_paths(ref.logformat)), name
    shape = rc.Shape(ref.parts)
    assert "".join(p[1] for p in shape.parts if p[0] == "lit") == "".join(shape.lits)
    e = emu.Emu(ref.logformat, ref.groups)
    assert e.status == 0, (name, e.status, e.err)


@pytest.mark.parametrize("name", rr.NAMES)
def test_handle_on_device(emu, name):
    e = emu.Emu(rr.logformat(name), rr.fields(name))
    assert e.status == 0, (name, e.status, e.err)


@pytest.mark.parametrize("name", rr.NAMES)
def test_reference_is_quick(oracle, name):
    """`re` alone over the corpus: a corpus on which a backtracking engine needs more than a few milliseconds per
    line (FORMAT_IP's nested {0,8}) is one to shrink.  Measured: about 5 microseconds per line."""
    c = rr.case(oracle, name)
    assert 2000 <= len(c.lines) <= 4000 and len(set(c.lines)) == len(c.lines)
    assert c.lines == rr.Case(oracle, name).lines  # deterministic
    t0 = time.perf_counter()
    for l in c.lines:
        c.expect(l)
    per_line = (time.perf_counter() - t0) / len(c.lines)
    print("%s: re %.1f us per line, %d lines of %.0f bytes" % (name, 1e6 * per_line, len(c.lines),
                                                               sum(map(len, c.lines)) / len(c.lines)))
    assert per_line < 2e-3, (name, per_line)


def fallback_cause(line):
    ctl = sorted({b for b in line if (b < 0x20 and b != 9) or b >= 0x7f})
    if ctl:
        return "bytes outside the device's text subset: " + " ".join("0x%02x" % b for b in ctl)
    return "the matcher leaves the priority among several ends of a list / IP token undecided"


@pytest.mark.parametrize("name", rr.NAMES)
def test_corpus_conditions(oracle, emu, name):
    """what the corpus must hold for the comparison to mean something, counted and asserted per handle: both
    outcomes, lines that need backtracking (the first DFS leaf fails, the line matches), lines that the prefilters
    pass and the DFS refuses, lines the prefilters alone rule out (all three from emu_leaf_stats on the format that
    matches, or on every format of the handle), and few FALLBACK lines (each printed with its cause)"""
    c = rr.case(oracle, name)
    emus = [emu.Emu(r.logformat, r.groups) for r in c.refs]
    n = len(c.lines)
    cnt = collections.Counter()
    for l, w in zip(c.lines, c.want):
        if w is not None:
            cnt["match"] += 1
            cnt["match " + emus[w[0]].leaf_class(l)] += 1
        else:
            cls = {e.leaf_class(l) for e in emus}
            assert "leaf" not in cls, (name, l)  # the first leaf is a match
            cnt["no match " + ("dfs" if "dfs" in cls else "prefilter")] += 1
    match, nomatch = cnt["match"], n - cnt["match"]
    e = emu.Emu(c.logformat, c.fields)
    fallback = [l for l in c.lines if e.parse_raw(l)[0] == EMU_FALLBACK]
    print("%s: %d lines; match %d (first leaf %d, backtracking %d); no match %d (DFS refuses %d, prefilters %d); "
          "FALLBACK %d" % (name, n, match, cnt["match leaf"], cnt["match dfs"], nomatch, cnt["no match dfs"],
                           cnt["no match prefilter"], len(fallback)))
    for l in fallback:
        print("  FALLBACK %r: %s" % (l, fallback_cause(l)))
    assert cnt["match prefilter"] == 0
    assert match >= 0.25 * n and nomatch >= 0.25 * n, cnt
    assert cnt["match dfs"] >= 0.10 * match, cnt
    assert cnt["no match dfs"] >= 0.05 * nomatch and cnt["no match prefilter"] >= 0.05 * nomatch, cnt
    assert len(fallback) <= 0.02 * n, (len(fallback), n)
    if len(c.refs) > 1:  # both formats of the handle are routed to, and often in turn
        routed = [w[0] for w in c.want if w is not None]
        assert min(routed.count(0), routed.count(1)) >= 0.2 * len(routed)
        assert sum(a != b for a, b in zip(routed, routed[1:])) >= 0.2 * len(routed)
    # the short lines (the GPU part's chunks of more than 64 lines) hold both outcomes too
    short = [c.expect(l) for l in c.short]
    assert sum(map(len, c.short)) / len(c.short) < 0.8 * sum(map(len, c.lines)) / n
    assert min(sum(w is not None for w in short), sum(w is None for w in short)) >= 0.2 * len(short)


def may_fall_back(c, line):
    """the lines the device may leave undecided (FALLBACK, whether they match or not): VT / FF bytes are outside
    its text subset, and the priority among the ends of an NGINX list token is not modelled.  Every other line of
    these corpora it has to decide."""
    lists = any(p[0] == "tok" and " *, *" in p[1] for r in c.refs for p in r.parts)
    return lists or b"\x0b" in line or b"\x0c" in line


def check(c, i, line, want, status, record, exact=True, more=False):
    """one line's status and record against `re`: no match <=> BAD; match => OK with every group's text; the
    device code only: FALLBACK where may_fall_back() allows it (counted by the caller: at most 2 % of a corpus).
    more: the handle has further paths requested (STAGES); the record's other values are not looked at"""
    if status == EMU_FALLBACK and not exact:
        assert may_fall_back(c, line), (c.name, i, line, want)
        return 1
    if want is None:
        assert status == EMU_BAD, (c.name, i, line, status)
    else:
        assert status == EMU_OK, (c.name, i, line, want, status)
        rec = json.loads(record)
        if more:
            rec = {k: v for k, v in rec.items() if k in c.fields}
        assert c.same(want, rec), (c.name, i, line, c.record(want), record)
    return 0


# With exactly the groups' paths requested a handle has no time and no first-line stage, and the chunk kernel's
# fixed-shape instances (lp_fixed.h) are picked only for the program that has both.  These two paths add them to
# common / combined; every timestamp of the corpora is a valid date and a first line that is none gives no method,
# so the statuses stay the regex's.
STAGES = ["TIME.EPOCH:request.receive.time.epoch", "HTTP.METHOD:request.firstline.method"]


@pytest.mark.parametrize("name", ["combined", "common"])
def test_emulation_with_stages(oracle, emu, name):
    """common / combined as the fixed-shape instances see them (STAGES requested too): the same statuses and
    group texts, the same FALLBACK lines; and the oracle agrees that no stage fails a matching line"""
    c = rr.case(oracle, name)
    e, e0 = emu.Emu(c.logformat, c.fields + STAGES), emu.Emu(c.logformat, c.fields)
    o = oracle.Oracle(c.logformat, c.fields + STAGES)
    for i, (l, w) in enumerate(zip(c.lines, c.want)):
        st, js = e.parse_raw(l)
        assert check(c, i, l, w, st, js, exact=False, more=True) == (e0.parse_raw(l)[0] == EMU_FALLBACK)
        so, jo = o.parse_raw(l)
        if so != oracle.UNSUPPORTED:
            check(c, i, l, w, so, jo, more=True)


@pytest.mark.parametrize("name", rr.NAMES)
def test_oracle_against_re(oracle, name):
    """the oracle (jregex.c) against `re` on every line; UNSUPPORTED only for the VT / FF lines"""
    c = rr.case(oracle, name)
    o = oracle.Oracle(c.logformat, c.fields)
    assert len(c.refs) > 1 or o.regex() == c.refs[0].java
    for i, (l, w) in enumerate(zip(c.lines, c.want)):
        st, js = o.parse_raw(l)
        if st == oracle.UNSUPPORTED:
            assert b"\x0b" in l or b"\x0c" in l, (name, l)
            continue
        check(c, i, l, w, st, js)


@pytest.mark.parametrize("name", rr.NAMES)
def test_emulation_against_re(oracle, emu, name):
    """the device per-line code on the CPU (both scanner modes) against `re`: line by line, and with the lines
    in one buffer among their neighbours (parse_batch_raw); the same lines FALLBACK either way"""
    c = rr.case(oracle, name)
    e = emu.Emu(c.logformat, c.fields)
    assert e.status == 0, e.err
    fb = []
    for i, (l, w) in enumerate(zip(c.lines, c.want)):
        st, js = e.parse_raw(l)
        if check(c, i, l, w, st, js, exact=False):
            fb.append(i)
    e = emu.Emu(c.logformat, c.fields)
    got = e.parse_batch_raw(b"".join(l + b"\n" for l in c.lines))
    assert len(got) == len(c.lines)
    fb2 = [i for i, (st, js) in enumerate(got) if check(c, i, c.lines[i], c.want[i], st, js, exact=False)]
    assert fb == fb2
    assert len(fb) <= 0.02 * len(c.lines)
    got = emu.Emu(c.logformat, c.fields).parse_batch_raw(b"".join(l + b"\n" for l in c.short))
    for i, (st, js) in enumerate(got):
        check(c, i, c.short[i], c.expect(c.short[i]), st, js, exact=False)
