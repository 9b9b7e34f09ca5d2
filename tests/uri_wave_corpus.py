"""Seeded boundary corpora for the wave-cooperative code of the URI kernels
(uri.hip: the 16-byte-block gather of uri_compact, the three path tiers,
uri_walk_coop, the spread query-piece pass of uri_wave), shared by
test_uri_wave.py (CPU emulation, which also validates the corpora) and
test_uri_wave_gpu.py.

Lines are built from explicit parts, so a generator knows each URI span's byte
offset in the batch buffer, its length, and the number of event bytes in it:
event bytes are % & ? + # ; and the bytes URIUtil escapes (| ^ { } ` < >);
everything else in a URI is drawn from [a-z0-9/._=-].  All lines stay inside
the device subset (ASCII, bad escapes only of class R1 of uri_repair_corpus,
no entities): none may be FALLBACK.

A family function returns Cases; a Case is one batch buffer with what the
generator knows about it."""
import random
import re

EVENTS = frozenset("%&?+#;|^{}`<>")
PW = 64  # lines per wave, events per walk round, pieces per block of the piece pass

HEAD = "10.1.2.3 - "
TS = "[10/Oct/2026:13:55:36 +0200]"
BAD_TS = "[10/Foo/2026:13:55:36 +0200]"  # BAD in phase 1: the line never reaches the URI kernels
REF_HOST = "http://h.example.com"


def count_events(uri):
    return sum(1 for c in uri if c in EVENTS)


def count_pieces(uri):
    """non-empty pieces of the raw query: from the first '&' / '?' to the first '#'"""
    m = re.search(r"[&?]", uri)
    if not m or "#" in uri[:m.start()]:
        return 0
    return sum(1 for p in re.split(r"[&?]", uri[m.end():].split("#", 1)[0]) if p)


class Case:
    """One batch: lines (each without its '\\n'), the buffer (default: every
    line terminated), per line the (request URI, referer) the generator planted
    (None: the line has none), the lines that are BAD in phase 1, the lines
    carrying a defect the device repairs."""

    def __init__(self, name, fmt="combined"):
        self.name, self.fmt = name, fmt
        self.lines, self.uris, self.spans = [], [], []
        self.bad, self.defective = set(), set()
        self.off = 0
        self.terminated = True
        self.info = {}

    def add(self, uri="/", referer="-", at=None, mod=16, bad=False, noreq=False, defect=False, agent="ua"):
        """at: the request URI starts at buffer offset `at` (mod `mod`), by
        padding the user field"""
        pre = len(HEAD) + 1 + len(BAD_TS if bad else TS) + len(' "GET ')
        user = "u"
        if at is not None and not noreq:
            user = "u" * (1 + (at - (self.off + pre + 1)) % mod)
        head = "%s%s %s " % (HEAD, user, BAD_TS if bad else TS)
        first = '""' if noreq else '"GET %s HTTP/1.1"' % uri
        mid = ' 200 %d "' % (100 + len(self.lines) % 900)
        l = head + first + mid + referer + '" "%s"' % agent
        a = self.off + len(head) + 5
        r = self.off + len(head) + len(first) + len(mid)
        self.spans.append((None if noreq else (a, a + len(uri)), None if referer == "-" else (r, r + len(referer))))
        self.uris.append((None if noreq else uri, None if referer == "-" else referer))
        k = len(self.lines)
        if bad:
            self.bad.add(k)
        elif defect:
            self.defective.add(k)
        self.lines.append(l.encode("ascii"))
        self.off += len(l) + 1
        return k

    def pad_wave(self):
        """lines without a URI up to the next multiple of 64 lines"""
        while len(self.lines) % PW:
            self.add(noreq=True)

    @property
    def data(self):
        d = b"\n".join(self.lines)
        return d + b"\n" if self.terminated else d

    # what the kernel derives, restated from the planted parts
    def wave_events(self, stage):
        """per wave, the event bytes of URI stage 0 (request) / 1 (referer) of its lines"""
        out = [0] * ((len(self.lines) + PW - 1) // PW)
        for k, u in enumerate(self.uris):
            if k not in self.bad and u[stage] is not None:
                out[k // PW] += count_events(u[stage])
        return out

    def wave_pieces(self):
        out = [0] * ((len(self.lines) + PW - 1) // PW)
        for k, u in enumerate(self.uris):
            if k not in self.bad and k not in self.defective:
                out[k // PW] += sum(count_pieces(x) for x in u if x is not None)
        return out

    def wave_blocks(self):
        """per wave, the aligned 16-byte blocks holding its lines' URI sources"""
        out = [0] * ((len(self.lines) + PW - 1) // PW)
        for k, s in enumerate(self.spans):
            s = [x for x in s if x is not None]
            if k in self.bad or not s:
                continue
            lo, hi = min(x[0] for x in s), max(x[1] for x in s)
            out[k // PW] += (((hi + 15) & ~15) - (lo & ~15)) >> 4
        return out

    def uri_bytes(self):
        return sum(b - a for k, s in enumerate(self.spans) if k not in self.bad for (a, b) in (x for x in s if x))


# ---------------------------------------------------------------- A: gather
def _sized_uri(n, tag):
    """a URI of exactly n bytes, with a short query when it fits"""
    if n < 8:
        return ("/" + "abcdefg")[:n]
    q = "?k7=%s" % tag
    q = q[:n - 2] if len(q) > n - 2 else q
    return "/" + "p" * (n - 1 - len(q)) + q


def gather_geometry(base=0):
    """A1: request URI start offset mod 16 x end offset mod 16 (all 256), plus
    spans of length 1, exactly one aligned block, and 17; every fourth line
    also has a referer with a query (a second source in the line's region).
    base: the buffer's own offset in a larger tensor (A4)."""
    c = Case("A1")
    for s in range(16):
        for e in range(16):
            n = 17 + (e - s - 17) % 16
            k = s * 16 + e
            ref = "-" if k % 4 else "%s/r%d?x=%d&y=a+b" % (REF_HOST, k % 7, k)
            c.add(_sized_uri(n, "v%d" % k), ref, at=(s - base) % 16)
    for s in range(16):
        c.add("/", at=s)
        c.add(_sized_uri(16, "w%d" % s), at=s)  # (s == 0: exactly one aligned block)
        c.add(_sized_uri(17, "x%d" % s), at=s)
    return c


def sparse_waves():
    """A2: waves in which few lanes, or none, have a URI"""
    full = lambda c, k: c.add("/s%d/x.html?k7=v%d&b=%%41+c" % (k, k), "%s/r?z=%d" % (REF_HOST, k))
    empty = lambda c, k: c.add(noreq=True) if k % 2 else c.add("/e%d?q=1" % k, bad=True)
    out = []
    for name, lanes in [("lane0", {0}), ("lane63", {63}), ("alternating", set(range(0, 64, 2))),
                        ("gap40", set(range(0, 12)) | set(range(52, 64))), ("none", set())]:
        c = Case("A2-" + name)
        for k in range(64):
            (full if k in lanes else empty)(c, k)
        c.info["uri_lanes"] = len(lanes)
        out.append(c)
    return out


def partial_last_block():
    """A3: the last line unterminated, its referer ending 4-5 bytes before the
    end of the buffer (the closest 'combined' allows: '" "' + agent + '"'), one
    buffer per nbytes % 16: the gather's last block is partial"""
    out = []
    for m in range(16):
        c = Case("A3-%d" % m)
        c.terminated = False
        for k in range(5):
            c.add("/a%d?k7=%d" % (k, k), "%s/r?z=%d" % (REF_HOST, k))
        agent = "a" * (m % 2)
        ref = REF_HOST + "/last?q=%41&k7=z"
        rest = len(' HTTP/1.1" 200 105 "') + len(ref) + len('" "') + len(agent) + 1
        pre = len(HEAD) + 2 + len(TS) + len(' "GET ')
        n = (m - (c.off + pre + rest)) % 16 + 16
        k = c.add(_sized_uri(n, "end"), ref, agent=agent)
        assert len(c.data) % 16 == m and len(c.data) - c.spans[k][1][1] == 4 + m % 2
        out.append(c)
    return out


# ------------------------------------------------------------ B: path tiers
def wave_with_total(T, variant=None):
    """One 64-line wave whose request URIs hold T bytes in all (T a multiple
    of 16): equal clean URIs of a multiple of 16 bytes, the last line absorbing
    the remainder; every URI starts block-aligned, so the wave's block total
    is T / 16, monotone in T.
    variant "long": line 7 takes a URI of 6400 bytes out of T; "defect": an R1
    defect in lanes 0, 31 and 63."""
    assert T % 16 == 0
    c = Case("B-%d%s" % (T, "-" + variant if variant else ""))
    big = 6400 if variant == "long" else 0
    n = max(16, (T - big) // 1024 * 16)
    sizes = [n] * 63 + [T - big - n * (62 if big else 63)]
    if big:
        sizes[7] = big
    assert 16 <= sizes[63] < 8000, (T, variant)
    for k, sz in enumerate(sizes):
        bad = variant == "defect" and k in (0, 31, 63)
        tail = "&x=50%-off" if bad else ""
        q = "/w?k7=%d&n=" % k
        body = q + "v" * (sz - len(q) - len(tail)) + tail
        assert len(body) == sz, (T, variant, k)
        c.add(body, at=0, defect=bad)
    assert c.uri_bytes() == T and c.wave_blocks() == [T // 16]
    return c


# ------------------------------------------------- C: list / pair tokens (lin)
def cookie_wave(uri_total, tok_len):
    """COOKIE_FMT lines: 64 request URIs of uri_total bytes in all, each line
    with a Cookie header of tok_len bytes whose values need decoding"""
    c = Case("C-cookie-%d" % tok_len, fmt="cookie")
    for k in range(64):
        ck = "S=%%41+c; p%d=" % k
        assert tok_len >= len(ck)
        ck += "x" * (tok_len - len(ck))
        c.lines.append(('10.1.2.3 - - %s "GET %s HTTP/1.1" 200 5 "%s"'
                        % (TS, _sized_uri(uri_total // 64, "c%d" % k), ck)).encode("ascii"))
    return c


def upstream_wave(uri_total, tok_len):
    """UPSTREAM_FMT lines: the $upstream_addr list swept in length"""
    c = Case("C-upstream-%d" % tok_len, fmt="upstream")
    for k in range(64):
        items = ["10.0.%d.0:80" % k]
        while len(", ".join(items)) < tok_len:
            items.append("10.0.%d.%d:80" % (k, len(items)))
        c.lines.append(('1.2.3.4 "%s" %s \\x01\\x02\\x03\\x04 "GET %s HTTP/1.1"'
                        % (", ".join(items), "200",  # (an unquoted status list with blanks is not decided on the device)
                           _sized_uri(uri_total // 64, "u%d" % k))).encode("ascii"))
    return c


# ------------------------------------------------------ D: cooperative walk
_PRE = ["|a", "+b", "%41c", "^", "{d", "}e", "`", "<f", ">g"]            # before the first separator
_POST = ["&a%d=b", "+w", "%%41", "&", "&=v%d", "&c%d=", "&d==e", "?x=%d", "|", "&Up%d=X", "&k7=%d", "^q", "%%7Eh",
         "&f", "+", "+2"]                                           # one event byte each


def ev_uri(rng, k, pre=0, tail=""):
    """a URI with exactly k event bytes: pre of them before the first '?'
    (escaped bytes, '+', valid escapes), then '?', then pieces; tail is
    appended as it is (its event bytes count)"""
    k -= count_events(tail)
    assert k >= 0 and (pre < k or k == 0 or pre == k)
    if k == 0:
        return "/plain/path-%d.html" % rng.randrange(100) + tail
    s = "/p" + "".join(rng.choice(_PRE) for _ in range(min(pre, k)))
    if pre < k:
        s += "?a=%d" % rng.randrange(10)
        for _ in range(k - pre - 1):
            a = rng.choice(_POST)
            s += a % rng.randrange(10) if "%d" in a else a.replace("%%", "%")
    s += tail
    return s


def _emit(c, uri, where, defect=False):
    if where == "req":
        return c.add(uri, defect=defect)
    if where == "ref":
        return c.add("/", REF_HOST + uri, defect=defect)
    return c.add(uri, REF_HOST + uri, defect=defect)


def _cur_blocks(c):
    """blocks of the current, partial wave"""
    return c.wave_blocks()[-1] if len(c.lines) % PW else 0


WALK_K = (0, 1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 200)


def walk_positions(seed=7, where="req", step=1):
    """D1: a line of every k of WALK_K starting at every position of a round
    (a filler line before it brings the wave's event count there), so lines
    span two and three rounds at every phase; zero-event lanes before, between
    and after (lines without a URI, and URIs without an event)."""
    rng = random.Random(seed)
    c = Case("D1-" + where)
    e, n = 0, 0
    for pos in range(0, 64, step):
        for k in WALK_K[1:]:
            if len(c.lines) % PW > 60 or _cur_blocks(c) + k // 3 > 440:
                c.pad_wave()
            if len(c.lines) % PW == 0:
                e = 0
                c.add(noreq=True)
            f = (pos - e) % PW
            _emit(c, ev_uri(rng, f, pre=min(f, n % 3)) if f else "/zero", where)
            tail = ["", "z#frag", ".;x=1", ""][n % 4] if k > 2 else ""
            _emit(c, ev_uri(rng, k, pre=min(k, n % 4), tail=tail), where)
            if n % 2:
                c.add(noreq=True) if n % 4 == 1 else c.add("/none.html")
            e += f + k
            n += 1
    c.pad_wave()
    return c


def walk_totals(seed=8):
    """D2: waves whose event totals are exactly 64, 65, 128, 129 (and 63, 127)"""
    rng = random.Random(seed)
    c = Case("D2")
    for tot in (63, 64, 65, 127, 128, 129):
        parts = [tot // 2 - 3, 0, 3, tot - tot // 2]
        for p in parts:
            c.add(ev_uri(rng, p, pre=min(p, 1)))
        c.pad_wave()
    c.info["totals"] = [63, 64, 65, 127, 128, 129]
    return c


# (URI, defect): every event of each is placed as the last event of a round
# and as the first of the next
PLACED = [
    ("/p|x{y}^?a=1&b=2", False),                   # the first '?' after escaped bytes
    ("/p?a=1&bb=x%41y&c=3&dd=e+f&g=4", False),     # '%41' / '+' and its piece's closing '&'
    ("/p?&&a=&=v&a==b&x&", False),                 # empty pieces, a trailing '&'
    ("/p?&a=1", False),
    ("/p?a=1?b=2&c=3", False),                     # a second '?'
    ("/p`q?a=|1&b=^2&c={3}", False),               # escaped bytes before and after the first separator
    ("/p?a=1&b=2#frag", False),                    # stop events
    ("/p?a=1&bcd#f?g&h", False),
    ("/p?a=1&b=2.;c=3&d=4", False),
    ("/p.;v=1?a=1&b=2", False),
    ("/p?a=1&b=%zz&c=1", True),
    ("/p?a=1&b=x%", True),                         # '%' at b-1, b-2, b-3
    ("/p?a=1&b=x%4", True),
    ("/p?a=1&b=x%4g", True),
    ("/p?a=1&b=x%41", False),                      # a valid escape ending exactly at b
    ("/p&a=1&b=2+c", False),                       # the first separator a '&'
]


def walk_placed(seed=9, where="req"):
    """D3: filler lines put event j of each PLACED URI at round positions 63
    and 0, for every j"""
    rng = random.Random(seed)
    c = Case("D3-" + where)
    e = 0  # events of the current wave so far
    placed = []
    for uri, defect in PLACED:
        for j in range(count_events(uri)):
            for r in (63, 0):
                if len(c.lines) % PW > 61 or _cur_blocks(c) > 400:
                    c.pad_wave()
                if len(c.lines) % PW == 0:
                    e = 0
                f = (r - j - e) % PW
                _emit(c, ev_uri(rng, f, pre=min(f, 1)) if f else "/zero", where)
                _emit(c, uri, where, defect=defect)
                placed.append((len(c.lines) - 1, j, (e + f + j) % PW))
                e += f + count_events(uri)
    c.info["placed"] = placed
    return c


def amp_runs(where="req"):
    """D4: a URI with 130 consecutive '&' at all 64 offsets mod 64 of the
    compact buffer (UEV bits on bit 63 and bit 0 of a mask word, the search
    crossing words): after a line whose region is 0..3 blocks, at each start
    offset mod 16"""
    c = Case("D4-" + where)
    uri = "/p?a=1" + "&" * 130 + "b=2&c"
    # a referer starts this far after the block-relative start of its line's region
    delta = 0 if where == "req" else len('/ HTTP/1.1" 200 123 "') + len(REF_HOST)
    for r in range(64):
        if len(c.lines) % PW > 60:
            c.pad_wave()
        at = (r - delta) % 16
        nb = ((r - at - delta) // 16 - _cur_blocks(c)) % 4
        if nb:
            c.add(_sized_uri(16 * nb - 3, "p"), at=0)
        else:
            c.add(noreq=True)
        if where == "req":
            c.add(uri, at=at)
        else:
            c.add("/", REF_HOST + uri, at=at)
    c.info["uri"] = uri
    return c


def amp_run_offsets(c):
    """the compact-buffer offsets mod 64 at which D4's runs of '&' start"""
    out, first = set(), 0
    for k, s in enumerate(c.spans):
        if k % PW == 0:
            first = 0
        s = [x for x in s if x is not None]
        if not s:
            continue
        lo, hi = min(x[0] for x in s), max(x[1] for x in s)
        for u, sp in zip(c.uris[k], c.spans[k]):
            if u and "&&&" in u:
                out.add((16 * first + sp[0] + u.index("&&&") - (lo & ~15)) % 64)
        first += (((hi + 15) & ~15) - (lo & ~15)) >> 4
    return out


def walk_cases():
    out = [walk_positions(7, "req"), walk_positions(17, "ref", step=4), walk_positions(27, "both", step=8), walk_totals()]
    out += [walk_placed(9, w) for w in ("req", "ref", "both")]
    out += [amp_runs("req"), amp_runs("ref")]
    return out


# ---------------------------------------------------------- E: piece pass
_NAMES = ["k7", "a", "Upper", "K7", "n|m", "b%41c", "x", "zz9"]
_VALUES = ["", "v", "%41", "a+b", "%41%42x", "x%7Ey+", "plain", "w+%2F"]  # decoded lengths 0, 1, 1, 3, 3, 4, 5, 3


def _piece(i):
    """the i-th non-empty piece: plain, upper-case names, names with escaped
    bytes, values with %XX / '+', no '='"""
    name = _NAMES[i % len(_NAMES)] if i % 5 else "k7"
    if i % 11 == 3:
        return name.replace("|", "")  # no '='
    return name + "=" + _VALUES[(i // 3) % len(_VALUES)]


def _query(n, start):
    return "&".join(_piece(start + j) for j in range(n))


PIECE_TOTALS = sorted(set(list(range(1, 9)) + list(range(8, 705, 37)) +
                          [m + d for m in range(64, 705, 64) for d in (-1, 0, 1)]))


def piece_counts(p):
    """pieces per line of a wave with p pieces: skewed (one line with up to
    300, the others 0-3)"""
    counts, left = [], p
    for c0 in (3, 0, 2):
        n = min(c0, left)
        counts.append(n)
        left -= n
    if left > 8:
        n = min(300, left - 5)
        counts.append(n)
        left -= n
    pat = (1, 0, 3, 2)
    while left and len(counts) < 60:
        n = min(pat[len(counts) % 4], left)
        counts.append(n)
        left -= n
    while left:
        n = min(left, 300)
        counts.append(n)
        left -= n
    assert len(counts) <= 64 and sum(counts) == p
    return counts


def piece_wave(c, p):
    """appends one wave with p pieces in all, request and referer stages summed"""
    start = p
    for n in piece_counts(p):
        ref = n // 3
        req = n - ref
        uri = "/q%d" % (p % 10) + ("?" + _query(req, start) if req else "")
        referer = REF_HOST + "/r" + ("?" + _query(ref, start + req) if ref else "")
        c.add(uri, referer if n % 2 or ref else "-")
        start += n
    c.pad_wave()


def piece_cases(totals=PIECE_TOTALS, chunk=12):
    out = []
    for i in range(0, len(totals), chunk):
        c = Case("E-%d" % totals[i])
        for p in totals[i:i + chunk]:
            piece_wave(c, p)
        c.info["totals"] = list(totals[i:i + chunk])
        out.append(c)
    return out


NAMED_FIELDS = ["STRING:request.firstline.uri.query.k7", "HTTP.PATH:request.referer.path"]


# ------------------------------------------------------- F: wave activity
def activity_cases(seed=5):
    out = []
    for n in (1, 63, 64, 65, 127, 128, 129):
        rng = random.Random(seed + n)
        c = Case("F-%d" % n)
        for k in range(n):
            ev = WALK_K[k % 8] if k % 7 else 66
            c.add(ev_uri(rng, ev, pre=min(ev, k % 3), tail="z#f" if k % 5 == 4 and ev > 2 else ""),
                  REF_HOST + ev_uri(rng, k % 4) if k % 2 else "-", bad=k % 3 == 2)
        out.append(c)
    return out


# ------------------------------------------------------ G: several formats
_REQ = re.compile(rb'"([A-Z]+) (\S+) (HTTP/[0-9.]+)"')
_REF = re.compile(rb'" \d+ \S+ "(http[^"]*)"')


def mixed_case(lines, seed=6):
    """lines: a corpus of several LogFormats (mixed_lines of test_emu_parity);
    request URIs and referers replaced by D- and E-style ones"""
    rng = random.Random(seed)
    c = Case("G", fmt="mixed")
    for k, l in enumerate(lines):
        m = _REQ.search(l)
        if m and k % 4 != 3:
            uri = ev_uri(rng, WALK_K[k % 9], pre=k % 3) if k % 2 else "/g?" + _query(k % 23, k)
            l = l[:m.start(2)] + uri.encode("ascii") + l[m.end(2):]
        m = _REF.search(l)
        if m and k % 3 == 0:
            ref = REF_HOST + (ev_uri(rng, (k // 3) % 70) if k % 2 else "/h?" + _query(k % 17, k + 5))
            l = l[:m.start(1)] + ref.encode("ascii") + l[m.end(1):]
        c.lines.append(l)
    return c
