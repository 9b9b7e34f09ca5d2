"""The straight-line first leaf of the fixed-shape instances (lp_device.h
fixed_fast_leaf) on the CPU (tests/emu/fixed_fast_emu.cpp): it may only
accept, with exactly the generic first leaf's spans; the instance's first leaf
and whole phase 1 equal the generic ones on every line of the corpus at every
window offset; and nearly every line of the flagship workload takes it."""
import os
import re
import subprocess

import pytest

import fixed_fast_corpus as corpus
import fixed_fast_emu_lib as ff
import logparser_amd as lpa

SHAPES = ("combined", "common")


@pytest.fixture(scope="module")
def fast():
    return {name: ff.Fast(name) for name in SHAPES}


def to_common(line):
    """the common-format part of a combined line"""
    return line.rsplit(b' "', 2)[0]


def test_limits_are_the_corpus_limits():
    assert ff.limits() == (corpus.HEAD, corpus.TAIL, corpus.DIGITS, corpus.STATUS)


# ------------------------------------------------- the corpus, from its bytes
def ws_positions(line):
    return [i for i, c in enumerate(line) if c <= 0x20]


def quote_positions(line):
    return [i for i, c in enumerate(line) if c == 0x22]


def test_corpus_holds_the_edge_cases():
    """re-derived from the bytes, not from the case names"""
    comb = corpus.lines("combined")
    comm = corpus.lines("common")
    edges_head = {64 * w + b for w in range(corpus.HEAD // 64) for b in corpus.EDGE_BITS}
    edges_tail = {corpus.TAIL - (64 * w + b) for w in range(corpus.TAIL // 64) for b in corpus.EDGE_BITS}
    for ls in (comb, comm):
        first = {k: set() for k in range(3)}
        for l in ls:
            for k, p in enumerate(ws_positions(l)[:3]):
                first[k].add(p)
        assert edges_head <= first[0]                       # the first separator on every edge bit (0 included)
        assert {e for e in edges_head if e >= 2} <= first[1]
        assert {e for e in edges_head if e >= 4} <= first[2]
        assert {corpus.HEAD - 1, corpus.HEAD, corpus.HEAD + 1} <= first[2]   # the head limit
        lens = {len(l) for l in ls}
        for n in (corpus.HEAD, corpus.TAIL, 512, corpus.MAX_LINE):
            assert {n - 1, n, n + 1} <= lens
        assert any(b"\t" in l for l in ls) and any(l.endswith(b"\r") for l in ls) and any(b"  " in l for l in ls)
    # distances of the last and the fifth quote from the end (combined), of the last one (common)
    d2, d5 = set(), set()
    for l in comb:
        q = quote_positions(l)
        if len(q) >= 6 and q[-1] == len(l) - 1:
            d2.add(len(l) - q[-2])
            d5.add(len(l) - q[-5])
    assert {d for d in edges_tail if d >= 2} <= d2
    assert {d for d in edges_tail if d >= 13} <= d5
    assert {corpus.TAIL - 1, corpus.TAIL, corpus.TAIL + 1, corpus.TAIL + 2} <= d5   # the tail limit
    dl = {len(l) - quote_positions(l)[-1] for l in comm if quote_positions(l)}
    assert {d for d in edges_tail if d >= 7} <= dl
    assert {corpus.TAIL, corpus.TAIL + 1} <= dl
    # quote counts after the request's start: fewer, exactly and more than the format's five
    counts = {len(quote_positions(l)) - 1 for l in comb}
    assert {3, 4, 5, 6, 7} <= counts and max(counts) >= 7
    names = [n for n, _ in corpus.cases("combined")]
    assert len(names) == len(set(names))


# -------------------------------------------------------------- differential
@pytest.mark.parametrize("name", SHAPES)
def test_corpus_every_window_offset(fast, name):
    ls = corpus.lines(name)
    n, st, flags, first = fast[name].run(ls, ff.ALL_OFFSETS)
    assert n == 0, (first, st)
    assert st["views"] == 64 * len(ls)
    assert st["offset_dependent"] == 0, st     # the limits are relative to the line, not to its window
    assert st["fast"] > 0 and st["walked"] > 0 and st["ok"] > 0 and st["bad"] > 0 and st["redo"] > 0 and st["fallback"] > 0, st
    # a line the fast leaf takes is never one phase 1 stops before the match (too long, guard)
    assert st["fast"] >= st["views"] - st["walked"] - st["fallback"], st


@pytest.mark.parametrize("name", SHAPES)
def test_limits_decide_as_stated(fast, name):
    """the valid line stretched to each limit is accepted, one byte beyond it walks"""
    make = corpus.combined if name == "combined" else corpus.common
    by = dict(corpus.cases(name))
    n, st, flags, first = fast[name].run(list(by.values()))
    assert n == 0, first
    took = dict(zip(by.keys(), (int(f) & 1 for f in flags)))
    assert took[name + "/valid"] == 1
    assert took[name + "/s3@%d/long-u" % (corpus.HEAD - 1)] == 1 and took[name + "/s3@%d/long-u" % corpus.HEAD] == 0
    assert took[name + "/s3@%d/long-h" % (corpus.HEAD - 1)] == 1 and took[name + "/s3@%d/long-h" % corpus.HEAD] == 0
    assert took[name + "/num/b/" + "1" * corpus.DIGITS] == 1 and took[name + "/num/b/" + "1" * (corpus.DIGITS + 1)] == 0
    assert took[name + "/num/l/" + "1" * corpus.DIGITS] == 1 and took[name + "/num/l/" + "1" * (corpus.DIGITS + 1)] == 0
    assert took[name + "/status-len/%d" % (corpus.STATUS - 1)] == 1 and took[name + "/status-len/%d" % corpus.STATUS] == 0
    if name == "combined":
        assert took["combined/Q5-%d/long-ua" % corpus.TAIL] == 1 and took["combined/Q5-%d/long-ua" % (corpus.TAIL + 1)] == 0
        assert took["combined/Q5-%d/long-ref" % corpus.TAIL] == 1 and took["combined/Q5-%d/long-ref" % (corpus.TAIL + 1)] == 0
        for k in ("quotes4", "quotes3", "Q3+2!=Q2/x", "Q3+2!=Q2/2sp", "Q3+1/tab", "tab/rs", "tab/hl", "tail/b'\\r'"):
            assert took["combined/" + k] == 0, k
    else:
        # (the last quote is at most 2 + STATUS + DIGITS bytes before the end of an accepted common line)
        assert took["common/QL-%d" % corpus.TAIL] == 0 and took["common/QL-%d" % (corpus.TAIL + 1)] == 0
        for k in ("no-quote", "tab/rs", "tab/hl", "combined-line"):
            assert took["common/" + k] == 0, k


@pytest.fixture(scope="module")
def synth_lines():
    """the first 400 K lines of synthetic workload 2"""
    return lpa.synth(lpa.SYNTH_COMBINED, 20261015, 0, 400_000).split(b"\n")[:-1]


def test_flagship_lines_take_the_fast_leaf(fast, synth_lines):
    """fewer than 0.1 % of the first 400,000 workload-2 lines take the element walk"""
    assert len(synth_lines) == 400_000
    n, st, flags, first = fast["combined"].run(synth_lines)
    assert n == 0, (first, st)
    print("combined: %d of %d lines walked" % (st["walked"], st["views"]))
    assert st["ok"] == len(synth_lines) and st["walked"] + st["fast"] == len(synth_lines), st
    assert st["walked"] < 0.001 * len(synth_lines), st


def test_flagship_lines_as_common(fast, synth_lines):
    ls = [to_common(l) for l in synth_lines[:100_000]]
    n, st, flags, first = fast["common"].run(ls)
    assert n == 0, (first, st)
    assert st["ok"] == len(ls) and st["walked"] < 0.001 * len(ls), st


# ------------------------------------------------------- stand-alone programs
@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_standalone_program(tmp_path, sanitized):
    """the corpus at every window offset through a program with its own main,
    built plain and with -fsanitize=address,undefined, run directly"""
    exe = ff.build_main(sanitized)
    for name in SHAPES:
        path = os.path.join(str(tmp_path), name + ".txt")
        with open(path, "wb") as f:
            f.write(b"\n".join(corpus.lines(name)) + b"\n")
        r = subprocess.run([exe, name, path], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.search(r"(\d+) line views, 0 differ, (\d+) fast, (\d+) walked, 0 offset-dependent", r.stdout)
        assert m and int(m.group(1)) == 64 * len(corpus.lines(name)) and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout
