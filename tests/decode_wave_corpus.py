"""Corpora for the dense decode pass of the URI kernels' piece pass (uri.hip
uri_wave: a query value that holds a '%' / '+' is handed, by a descriptor in
LDS, to a lane of its own), shared by test_decode_wave.py (CPU emulation, which
also validates the corpora) and test_decode_wave_gpu.py.

The kernel numbers a wave's non-empty query pieces line after line (a line's
request-URI pieces, then its referer's), takes them in rounds of 4 blocks of
PW = 64 pieces, and decodes the waiting values whenever a block's would not
fit the CAPD descriptors of its buffer, and after a round's last block.  A
piece is "pv" when it has a '=' and a '%' or '+' after the first one: exactly
the pieces that get a descriptor when their name is requested.

Waves are built from explicit piece lists with uri_wave_corpus.Case, every
wave 64 lines, so a generator knows the index of every pv piece in its wave.
A Case's info["pv"] lists, per wave, the pv counts of its 64-piece blocks as
planted; wave_block_pv re-derives them from the URIs."""
import re

import uri_wave_corpus as uwc
from uri_wave_corpus import PW, REF_HOST, Case

CAPD = 64  # uri.hip URI_CAPD: descriptors the buffer holds
ROUND = 4 * PW  # pieces per round (LP_URI_QR blocks)


def piece_flags(uri):
    """per non-empty piece of the raw query (uri_wave_corpus.count_pieces):
    whether its value needs decoding"""
    m = re.search(r"[&?]", uri)
    if not m or "#" in uri[:m.start()]:
        return []
    out = []
    for p in re.split(r"[&?]", uri[m.end():].split("#", 1)[0]):
        if p:
            out.append("=" in p and bool(re.search(r"[%+]", p.split("=", 1)[1])))
    return out


def count_pv(uri):
    return sum(piece_flags(uri))


def wave_block_pv(case):
    """per wave, the pv pieces of each 64-piece block, from the planted URIs"""
    out = []
    for w in range(0, len(case.lines), PW):
        flags = []
        for k in range(w, min(w + PW, len(case.lines))):
            if k in case.bad or k in case.defective:
                continue
            for u in case.uris[k]:
                if u is not None:
                    flags += piece_flags(u)
        out.append([sum(flags[b:b + PW]) for b in range(0, len(flags), PW)])
    return out


# ------------------------------------------------------------ building waves
_PLAIN_NAMES = ["a", "k7", "x", "zz9"]
_PV_NAMES = ["k7", "b", "k7", "q"]
_PV_VALUES = ["a+b", "%41", "x%7Ey+", "+", "%41%42x", "w+%2F"]


def plain_piece(i):
    return "%s=v%d" % (_PLAIN_NAMES[i % 4], i % 10)


def pv_piece(i):
    return "%s=%s" % (_PV_NAMES[i % 4], _PV_VALUES[i % len(_PV_VALUES)])


def pieces_with(n, pv_at):
    """n pieces, the ones at the indices pv_at pv, the others plain"""
    pv_at = set(pv_at)
    return [pv_piece(i) if i in pv_at else plain_piece(i) for i in range(n)]


def _blocks(flags):
    return [sum(flags[b:b + PW]) for b in range(0, len(flags), PW)]


def add_wave(c, pieces, per_line=None, where="req"):
    """appends one 64-line wave holding `pieces` in order: per_line pieces in
    each line's request URI (where="req"), referer ("ref"), or the first half
    in the request URI and the rest in the referer ("both"); default: spread
    over all 64 lines.  Notes the planted pv counts per block."""
    assert len(c.lines) % PW == 0
    n0 = len(c.lines)
    per_line = per_line or max(1, (len(pieces) + PW - 1) // PW)
    for i in range(0, len(pieces), per_line):
        ch = pieces[i:i + per_line]
        if where == "req":
            c.add("/d%d?" % (i % 7) + "&".join(ch))
        elif where == "ref":
            c.add("/", REF_HOST + "/r?" + "&".join(ch))
        else:
            h = (len(ch) + 1) // 2
            c.add("/d?" + "&".join(ch[:h]), REF_HOST + "/r" + ("?" + "&".join(ch[h:]) if ch[h:] else ""))
    assert pieces and n0 < len(c.lines) <= n0 + PW, (c.name, len(pieces), per_line)
    c.pad_wave()
    c.info.setdefault("pv", []).append(_blocks([bool(re.search(r"=.*[%+]", p)) for p in pieces]))


# ------------------------------------------------------------------ families
COUNTS = sorted({0, 1, 2, 63, 64, 65, CAPD - 1, CAPD, CAPD + 1, 128, 255, 256})


def count_cases():
    """N: n pv pieces, the first n of one 256-piece round, the others plain;
    and a block whose 64 pieces are all pv arriving when 1 descriptor waits"""
    c = Case("N-counts")
    for n in COUNTS:
        add_wave(c, pieces_with(ROUND, range(n)))
    add_wave(c, pieces_with(ROUND, [17] + list(range(64, 128))))
    c.info["counts"] = COUNTS
    return c


def placement_cases():
    """P: where the pv pieces lie"""
    c = Case("P-placement")
    add_wave(c, pieces_with(ROUND, range(1, 64, 3)))            # every pv piece in block 0
    add_wave(c, pieces_with(ROUND, range(192, 256, 3)))         # ... in block 3
    add_wave(c, pieces_with(ROUND, (63, 127, 191, 255)))        # only in lane 63 of each block
    add_wave(c, pieces_with(300, range(0, 300, 5)), per_line=300)  # all in one 300-piece line
    for where in ("req", "ref", "both"):
        add_wave(c, pieces_with(ROUND, range(0, ROUND, 2)), where=where)
    # more than 256 pieces, the pv ones across the round boundary
    add_wave(c, pieces_with(320, range(250, 262)), per_line=5)
    add_wave(c, pieces_with(2 * ROUND + 10, list(range(192, 320)) + [2 * ROUND + 9]), per_line=9)
    return c


VALUES = ["+", "%41", "%E9", "%C3%A9", "%41%42%43", "%2B%2b", "++"] + \
         ["+" + "x" * (n - 1) for n in range(1, 10)] + ["y" * (n - 1) + "%7E" for n in range(1, 10)]


def value_cases():
    """V: what is decoded.  Each value ends at the URI's end, before a '&' and
    before a '#'."""
    c = Case("V-values")
    flags = []  # of the current wave's pieces, as planted
    c.info["pv"] = []
    for v in VALUES:
        if len(c.lines) % PW > PW - 3:
            c.pad_wave()
            c.info["pv"].append(_blocks(flags))
            flags = []
        c.add("/v?k7=" + v)
        c.add("/v?k7=%s&a=1" % v, REF_HOST + "/r?q=%s#f" % v)
        c.add("/v?x=1&k7=%s#frag" % v)
        flags += [True, True, False, True, False, True]
    c.pad_wave()
    c.info["pv"].append(_blocks(flags))
    return c


def long_value_case(n, path=1):
    """V: one n-byte value among 1-byte values in the same pass; path: the
    bytes of every line's path (they count towards the wave's URI bytes,
    which decide the tier the wave runs on)"""
    c = Case("V-long%d" % n)
    for i in range(PW):
        v = "a+%41b" * (n // 6) + "c" * (n % 6) if i == 7 else "+"
        c.add("/" + "p" * (path - 1) + "?k7=" + v)
    assert len(c.uris[7][0]) == path + 4 + n
    c.info["pv"] = [[PW]]
    return c


NAME_URIS = ["/n?Upper=%41", "/n?n|m=a+b", "/n?Upper=%41&n|m=a+b&k7=c+d", "/n?a|B=+&K7=%41&k7=%42", "/n?n|m=1&Upper=2&x=+"]


NAME_PV = [[True], [True], [True, True, True], [True, True, True], [False, False, True]]


def name_cases():
    """M: a rewritten name followed by a decoded value in one spill"""
    c = Case("M-names")
    flags = []
    for i in range(PW):
        u = NAME_URIS[i % len(NAME_URIS)]
        c.add(u, REF_HOST + u if i % 3 == 0 else "-")
        flags += NAME_PV[i % len(NAME_URIS)] * (2 if i % 3 == 0 else 1)
    c.info["pv"] = [_blocks(flags)]
    return c


def all_cases():
    return [count_cases(), placement_cases(), value_cases(), long_value_case(2000), long_value_case(6000, path=100), name_cases()]


NAMED_FIELDS = uwc.NAMED_FIELDS  # one named parameter (k7): the other pv pieces are skipped, nothing decoded


def mixed_decode_case(lines):
    """uri_wave_corpus.mixed_case over these URIs: the request URIs and
    referers of a corpus of several LogFormats replaced by the value and name
    families' and by rounds of pv pieces"""
    c = uwc.mixed_case(lines)
    uris = [u[0] for x in (value_cases(), name_cases()) for u in x.uris if u[0]]
    out = []
    for k, l in enumerate(c.lines):
        m = uwc._REQ.search(l)
        if m and k % 4 != 3:
            uri = uris[k % len(uris)] if k % 2 else "/g?" + "&".join(pieces_with(k % 23, range(0, k % 23, 2)))
            l = l[:m.start(2)] + uri.encode("ascii") + l[m.end(2):]
        m = uwc._REF.search(l)
        if m and k % 3 == 0:
            ref = REF_HOST + "/h?" + "&".join(pieces_with(k % 17, range(1, k % 17, 3)))
            l = l[:m.start(1)] + ref.encode("ascii") + l[m.end(1):]
        out.append(l)
    c.lines = out
    c.name = "G-decode"
    return c
