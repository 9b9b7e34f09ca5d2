"""Boundary batches for the owner lookup of the URI kernels' cooperative
passes (uri.hip OwnerRounds, lp_owner.h): which lane's line owns block /
event / piece g of the wave, from the round's head mask instead of a search.
Shared by test_uri_owner.py (CPU: validates the batches and their planted
quantities) and test_uri_owner_gpu.py.

A batch is one wave built from a PLAN: 64 per-lane item counts (blocks of the
gather, event bytes of the walk, query pieces of the piece pass).  A lane
with count 0 is, in turn, a line that is BAD in phase 1, a line without a
request, and (events / pieces) a line whose URI has no item.  Built with
uri_wave_corpus's Case and generators; lines stay inside the device subset."""
import random

from uri_wave_corpus import PW, REF_HOST, Case, count_events, count_pieces, ev_uri

URI_CAP = 8512           # uri.hip: the compact buffer of k_uri_lines (16 * blocks + 16 must fit)
FIRSTS = (63, 64, 65, 127, 128)


# ------------------------------------------------------------------- plans
def first_item_plan(T, run=0, edges=False):
    """(plan, target): lane `target`'s first item is exactly T, directly after
    `run` lanes without items; edges: lanes 0 and 63 have none either"""
    plan = [0] if edges else []
    plan += [70, T - 72, 2] if T > 100 else [T - 2, 2]
    plan += [0] * run
    target = len(plan)
    plan.append(3)
    plan += [1] * (PW - 1 - len(plan))
    plan.append(0 if edges else 2)
    assert len(plan) == PW and sum(plan[:target]) == T
    return plan, target


def long_lane_plan(lane, n):
    """one lane with n items (n > 64: a round without any head), the others one each"""
    plan = [1] * PW
    plan[lane] = n
    return plan, lane


def plans(long_n):
    """name -> (plan, target lane): the five first-item arrangements, the same
    with item-less lanes (0, 63, runs of 2 and 40 before the lane that starts
    on item 64), a long lane at 0 / 31 / 63, and 64 lanes of one item"""
    out = {"ones": ([1] * PW, 63)}
    for lane in (0, 31, 63):
        out["long%d" % lane] = long_lane_plan(lane, long_n)
    for T in FIRSTS:
        out["first%d" % T] = first_item_plan(T)
    for run in (2, 40):
        out["first64-run%d" % run] = first_item_plan(64, run, edges=True)
    return out


def firsts(plan):
    out, s = [], 0
    for n in plan:
        out.append(s)
        s += n
    return out


# ----------------------------------------------------------------- builders
def sized_uri(n, tag):
    """a URI of exactly n bytes, with a short query when it fits"""
    if n < 8:
        return ("/" + "abcdefg")[:n]
    q = ("?k7=%s" % tag)[:n - 2]
    return "/" + "p" * (n - 1 - len(q)) + q


def _no_item(c, k, plain=None):
    """the k-th item-less lane: BAD in phase 1, no request, or a URI without an
    item (the BAD line's URI has none either: with fields that leave the
    time stamp alone the line is OK, and still item-less)"""
    kind = k % (3 if plain else 2)
    if kind == 0:
        c.add(plain or "/b%d?x=1&y=2" % k, bad=True)
    elif kind == 1:
        c.add(noreq=True)
    else:
        c.add(plain)


def blocks_case(name, plan, target=None):
    """lane l's URI sources lie in plan[l] aligned 16-byte blocks: a request
    URI of 16 n bytes from a block boundary, a '-' referer"""
    c = Case("OB-" + name)
    for l, n in enumerate(plan):
        if n:
            c.add(sized_uri(16 * n, "b%d" % l), at=0)
        else:
            _no_item(c, l)
    c.info.update(space="blocks", plan=list(plan), target=target)
    return c


def line_blocks(c):
    """per line, the aligned 16-byte blocks holding its URI sources (the
    arithmetic of uri_wave_corpus's wave_blocks)"""
    out = []
    for k, s in enumerate(c.spans):
        s = [x for x in s if x is not None]
        if k in c.bad or not s:
            out.append(0)
            continue
        lo, hi = min(x[0] for x in s), max(x[1] for x in s)
        out.append((((hi + 15) & ~15) - (lo & ~15)) >> 4)
    return out


def events_case(name, plan, where, target=None, seed=11):
    """lane l's URI has plan[l] event bytes, in the request URI, the referer, or both"""
    rng = random.Random(seed + len(name))
    c = Case("OE-%s-%s" % (name, where))
    for l, n in enumerate(plan):
        if not n:
            _no_item(c, l, "/zero/path-%d.html" % l)
            continue
        uri = ev_uri(rng, n, pre=min(n, l % 3))
        if where == "req":
            c.add(uri)
        elif where == "ref":
            c.add("/", REF_HOST + uri)
        else:
            c.add(uri, REF_HOST + uri)
    c.info.update(space="events", plan=list(plan), where=where, target=target)
    return c


def line_events(c, stage):
    return [0 if k in c.bad or u[stage] is None else count_events(u[stage]) for k, u in enumerate(c.uris)]


_PIECES = ["k7=v%d", "a=%%41b", "Upper=x+y", "n%d", "k7=", "zz9=w+%%2F", "b=plain%d"]


def _query(n, start):
    return "&".join(p % (start + j) if "%d" in p else p.replace("%%", "%")
                    for j, p in ((j, _PIECES[(start + j) % len(_PIECES)]) for j in range(n)))


def pieces_case(name, plan, fmt="combined", target=None):
    """lane l's line has plan[l] query pieces: all in the request URI (even
    lanes), or a third of them in the referer (odd lanes).  fmt "mixed": the
    three-format handle; every third lane without a referer is a 'common' line."""
    c = Case("OP-%s%s" % (name, "-mixed" if fmt == "mixed" else ""), fmt=fmt)
    for l, n in enumerate(plan):
        if not n:
            _no_item(c, l, "/none-%d.html" % l)
            continue
        ref = n // 3 if l % 2 else 0
        uri = "/q%d?%s" % (l % 10, _query(n - ref, 7 * l))
        c.add(uri, REF_HOST + "/r?" + _query(ref, 7 * l + n) if ref else "-")
    if fmt == "mixed":
        for l, u in enumerate(c.uris):
            if l % 3 == 0 and u[0] is not None and u[1] is None and l not in c.bad:
                c.lines[l] = c.lines[l].rsplit(b' "', 2)[0]
    c.info.update(space="pieces", plan=list(plan), target=target)
    return c


def line_pieces(c):
    return [0 if k in c.bad else sum(count_pieces(x) for x in u if x is not None) for k, u in enumerate(c.uris)]


# -------------------------------------------------------------------- cases
def block_cases():
    """a URI of 1,056 bytes (66 blocks) for the long lane"""
    return [blocks_case(n, p, t) for n, (p, t) in plans(66).items()]


def block_overflow_case():
    """above URI_CAP: k_uri_overflow's buffer, its gather in two batches of
    nine rounds (637 blocks), lane 5 alone more than a round"""
    plan = [9] * PW
    plan[5] = 70
    c = blocks_case("overflow", plan)
    assert 16 * sum(plan) + 16 > URI_CAP
    return c


def event_cases(where):
    return [events_case(n, p, where, t) for n, (p, t) in plans(70).items()]


def piece_cases(fmt="combined"):
    return [pieces_case(n, p, fmt, t) for n, (p, t) in plans(70).items()]


def targets():
    """name -> (target lane, its first item) of the first-item arrangements"""
    out = {}
    for n, (p, t) in plans(66).items():
        if n.startswith("first"):
            out[n] = (t, firsts(p)[t])
    return out
