"""The lines of the regex-priority tests: for each format of regex_ref.FORMATS a deterministic, seeded corpus in
which the format's own separators occur inside the field values -- the lines on which the priority order of the
candidates, the pruning of greedy `.*` (need / kth_from_end), the literal-aware first candidates and the
quote-count / line-tail prefilters decide the outcome.

A corpus is built from the parts of the printed regex (regex_ref.split_regex) alone: the literals to plant and the
kind of every token come out of it, so a new format needs no hand work.  It knows nothing of what any engine
answers; regex_ref (Python's `re`) gives the expectation, test_regex_priority.py asserts the shares of matching,
backtracking and prefiltered lines the corpus must have.

Only ASCII, and of the controls only TAB and a few VT / FF (the other `\\s` bytes a line can hold; the device sends
them to FALLBACK by design): other controls, DEL and non-ASCII bytes are pinned elsewhere.  Every timestamp is a
valid date, so a regex match is never BAD for its time.
"""
import random

SEED = 20261021
N_LINES = 2600  # per format

_TIME_US = "[0-3][0-9]/(?:[a-zA-Z][a-zA-Z][a-zA-Z])/[1-9][0-9][0-9][0-9]:[0-9][0-9]:[0-9][0-9]:[0-9][0-9] [\\+|\\-][0-9][0-9][0-9][0-9]"
_TIME_ISO = "[1-9][0-9][0-9][0-9]-[0-1][0-9]-[0-3][0-9]T[0-9][0-9]:[0-9][0-9]:[0-9][0-9][\\+|\\-][0-9][0-9]:[0-9][0-9]"
_X = "[0-9]+\\.[0-9]+"
KINDS = {
    ".*?": "lazy", ".*": "greedy", "[^\\s]*": "nospace", "[0-9]+|-": "clfnum", "[0-9]+": "num",
    _TIME_US: "time_us", _TIME_ISO: "time_iso", _X: "decimal", "[0-9]+\\.[0-9][0-9][0-9]": "msec",
    "[^\\s]* [^\\s]* [^\\s]*": "request3",
    _X + "(?: *, *" + _X + "(?: *: *" + _X + ")?)*": "uplist_dec",
    "[^\\s]*(?: *, *[^\\s]*(?: *: *[^\\s]*)?)*": "uplist_ns",
}
FREE = ("lazy", "greedy", "nospace", "request3", "uplist_ns")  # the kinds whose values take planted text
NUMERIC = ("clfnum", "num", "decimal", "msec", "uplist_dec")

_WORDS = ["GET /index.html HTTP/1.1", "POST /a/b?x=1&y=2 HTTP/1.0", "http://example.com/p?q=1", "Mozilla/5.0 (X11; Linux)",
          "curl/8.1", "-", "", "a b c d", "k=v; s=t"]
_NOSPACE = ["200", "404", "frank", "1.2.3.4", "-", "", "x.example.com", "a=b"]
_SHORT_WORDS, _SHORT_NOSPACE = ["a b c", "-", "", "x"], ["2", "-", "", "f"]


def kind_of(token_regex):
    if token_regex not in KINDS:
        raise KeyError("regex_corpus knows no values for the token regex %r" % token_regex)
    return KINDS[token_regex]


class Shape:
    """a format's printed regex as the corpus sees it: literals and token kinds in order"""

    def __init__(self, parts):
        self.parts = [("lit", p[1]) if p[0] == "lit" else ("tok", kind_of(p[1])) for p in parts]
        self.lits = [p[1] for p in self.parts if p[0] == "lit"]
        self.toks = [i for i, p in enumerate(self.parts) if p[0] == "tok"]
        assert self.lits, "a format without literals"
        # every literal, every proper prefix and suffix of it
        frags = []
        for l in self.lits:
            for f in [l] + [l[:k] for k in range(1, len(l))] + [l[k:] for k in range(1, len(l))]:
                if f not in frags:
                    frags.append(f)
        self.frags = frags
        firsts = [l[0] for l in self.lits]
        self.byte = max(sorted(set(firsts)), key=firsts.count)  # the most frequent literal first byte
        # `need` of the greedy .* (csrc/lp_program.h): the copies of its literal's first byte in the literals from
        # there to the end; a format without one: the copies of `byte`
        self.need = "".join(self.lits).count(self.byte)
        for i in self.toks:
            if self.parts[i][1] == "greedy" and i + 1 < len(self.parts):
                self.need = "".join(p[1] for p in self.parts[i + 1:] if p[0] == "lit").count(self.parts[i + 1][1][0])
                self.byte = self.parts[i + 1][1][0]
                break

    def next_lit(self, i):
        return self.parts[i + 1][1] if i + 1 < len(self.parts) and self.parts[i + 1][0] == "lit" else ""


def base_value(kind, rng, short=False):
    if kind in ("lazy", "greedy"):
        return rng.choice(_SHORT_WORDS if short else _WORDS)
    if kind == "nospace":
        return rng.choice(_SHORT_NOSPACE if short else _NOSPACE)
    if kind == "clfnum":
        return rng.choice(["0", "5", "1234", "-", "98765"])
    if kind == "num":
        return rng.choice(["0", "5", "1234", "98765"])
    if kind == "time_us":
        return "%02d/%s/20%02d:%02d:%02d:%02d %s0%d00" % (rng.randrange(1, 29), rng.choice(["Jan", "Feb", "Oct", "Dec"]),
                                                         rng.randrange(10, 30), rng.randrange(24), rng.randrange(60),
                                                         rng.randrange(60), rng.choice("+-"), rng.randrange(10))
    if kind == "time_iso":
        return "20%02d-%02d-%02dT%02d:%02d:%02d%s0%d:00" % (rng.randrange(10, 30), rng.randrange(1, 13), rng.randrange(1, 29),
                                                           rng.randrange(24), rng.randrange(60), rng.randrange(60),
                                                           rng.choice("+-"), rng.randrange(10))
    if kind == "decimal":
        return rng.choice(["0.5", "12.345", "1.0"])
    if kind == "msec":
        return "%d.%03d" % (rng.randrange(1600000000, 1700000000), rng.randrange(1000))
    if kind == "request3":
        return rng.choice(["GET /index.html HTTP/1.1", "POST /a?x=1 HTTP/1.0", "HEAD / HTTP/2.0"])
    if kind == "uplist_dec":
        return rng.choice(["0.5", "1.5, 2.5", "1.5, 2.5 : 3.5", "0.001 : 0.002"])
    if kind == "uplist_ns":
        return rng.choice(["10.0.0.1:80", "10.0.0.1:80, 10.0.0.2:80", "a:1, b:2 : c:3", "-", "unix:/tmp/s"])
    raise KeyError(kind)


def planted(value, frag, where):
    mid = len(value) // 2
    if where == "start":
        return frag + value
    if where == "mid":
        return value[:mid] + frag + value[mid:]
    if where == "end":
        return value + frag
    return value[:mid] + frag + frag + value[mid:]  # twice in a row


NUMBER_EDGES = ["-", "-5", "5-", "", "007"]
DECIMAL_EDGES = ["1.", ".5", "1.23.4", "1.234", "1.2345", "12", "1.2", "-"]
REQUEST_EDGES = ["GET /x", "GET /x HTTP/1.1", "GET /x y HTTP/1.1", 'GET /x HT"TP', 'GET /x HTTP/1.1"', 'GET "/x" HTTP/1.1',
                 "GET  HTTP/1.1", "  ", " /x ", "GET\t/x HTTP/1.1"]


def uplist_edges():
    out = []
    for a in range(3):
        for b in range(3):
            out.append("1.5" + " " * a + "," + " " * b + "2.5" + " " * b + ":" + " " * a + "3.5")
    out += ["1.5, 2.5, ", "1.5, - : 3.5", "-", "1.5,2.5:3.5:4.5", "1.5 2.5", "1.5, 2.5 :", "1.5 , 2", "1.5, 2.5 : 3.5, 4.5 : 5.5"]
    return out


class Builder:
    def __init__(self, shape, seed, short=False):
        self.s = shape
        self.short = short
        self.rng = random.Random(seed)
        self.lines = []
        self.seen = set()

    def values(self):
        return {i: base_value(self.s.parts[i][1], self.rng, self.short) for i in self.s.toks}

    def join(self, vals, lits=None):
        out, k = [], 0
        for i, p in enumerate(self.s.parts):
            if p[0] == "lit":
                out.append(p[1] if lits is None else lits[k])
                k += 1
            else:
                out.append(vals[i])
        return "".join(out)

    def add(self, line):
        if "\n" in line or "\r" in line or line in self.seen:
            return
        self.seen.add(line)
        self.lines.append(line.encode("ascii"))

    def toks_of(self, kinds):
        return [i for i in self.s.toks if self.s.parts[i][1] in kinds]

    # ---- the systematic part
    def plain(self, n):
        for _ in range(n):
            self.add(self.join(self.values()))

    def separators(self):
        """every literal and every proper prefix / suffix of it inside each free-text field: at its start, middle
        and end and twice in a row"""
        for i in self.toks_of(FREE):
            for frag in self.s.frags:
                for where in ("start", "mid", "end", "twice"):
                    v = self.values()
                    v[i] = planted(v[i], frag, where)
                    self.add(self.join(v))

    def need_copies(self):
        """0..6 and need-1, need, need+1, need+5 extra copies of the literal first byte that `need` counts, alone
        and with the rest of that literal, in each field that takes text"""
        s = self.s
        counts = sorted({k for k in list(range(7)) + [s.need - 1, s.need, s.need + 1, s.need + 5] if k >= 0})
        lit = next((l for l in s.lits if l[0] == s.byte and len(l) > 1), s.byte)
        for i in self.toks_of(("lazy", "greedy")):
            for k in counts:
                for unit in (s.byte, lit, s.byte + "x"):
                    v = self.values()
                    v[i] = planted(v[i], unit * k, "mid")
                    self.add(self.join(v))
                    v = self.values()
                    for j in self.toks_of(("lazy", "greedy")):  # spread over the text fields
                        v[j] = planted(v[j], unit * (k // 2 + (j == i) * (k % 2)), "end")
                    self.add(self.join(v))

    def lazy_greedy(self):
        """the fields behind .*? and .* each hold the separator that follows them; all of them at once too"""
        ts = self.toks_of(("lazy", "greedy"))
        for where in ("start", "mid", "end", "twice"):
            v = self.values()
            for i in ts:
                v[i] = planted(v[i], self.s.next_lit(i), where)
            self.add(self.join(v))
            for i in ts:
                for j in ts:
                    if i < j:
                        v = self.values()
                        v[i] = planted(v[i], self.s.next_lit(i), where)
                        v[j] = planted(v[j], self.s.next_lit(j), where)
                        self.add(self.join(v))

    def straddles(self, g):
        """[(token j, text a)]: the separator after the text field g as `a` at the end of a later field j plus the
        start of j's own separator -- a candidate of g that no field contains (common: a status that ends in '"')"""
        lg = self.s.next_lit(g)
        out = []
        for j in self.s.toks:
            lj = self.s.next_lit(j)
            if j <= g or not lj:
                continue
            for k in range(1, len(lg)):
                a, b = lg[:k], lg[k:]
                if (lj.startswith(b) or b.startswith(lj)) and self.s.parts[j][1] in FREE + ("clfnum", "num"):
                    out.append((j, a))
        return out

    def decoys(self, reps):
        """a later, false candidate for each text field's separator: straddling a later field's end, with 0..3 more
        copies of the separator inside the field itself"""
        for g in self.toks_of(("lazy", "greedy")):
            lg = self.s.next_lit(g)
            for j, a in self.straddles(g):
                for r in range(reps):
                    v = self.values()
                    v[j] = v[j] + a
                    for _ in range(r % 4):
                        v[g] = planted(v[g], lg, self.rng.choice(("start", "mid", "end")))
                    self.add(self.join(v))

    def numbers(self):
        for i in self.toks_of(("clfnum", "num")):
            nxt = self.s.next_lit(i)[:1]
            for e in NUMBER_EDGES + ["12" + nxt + "34", "12" + nxt, nxt + "12"]:
                for _ in range(3):
                    v = self.values()
                    v[i] = e
                    self.add(self.join(v))
        for i in self.toks_of(("decimal", "msec")):
            for e in DECIMAL_EDGES:
                for _ in range(3):
                    v = self.values()
                    v[i] = e
                    self.add(self.join(v))

    def uplists(self):
        for i in self.toks_of(("uplist_dec", "uplist_ns")):
            for e in uplist_edges():
                nxt = self.s.next_lit(i)
                # ... followed by a digit-led and a non-digit-led text, and by its separator and one more item
                for tail in ("", nxt[:1] + "7", nxt[:1] + "x", nxt + "2.5", nxt + "2.5" + nxt + "x"):
                    v = self.values()
                    v[i] = e + tail
                    self.add(self.join(v))

    def requests(self):
        for i in self.toks_of(("request3",)):
            nxt = self.s.next_lit(i)
            for e in REQUEST_EDGES + ["GET /x H" + nxt[:1], "GET /x H" + nxt + "T", "GET " + nxt + " H"]:
                for _ in range(3):
                    v = self.values()
                    v[i] = e
                    self.add(self.join(v))

    def line_ends(self):
        """lines that stop directly before, inside and directly after each literal (the last one among them), and
        trailing bytes after a complete match"""
        for _ in range(3):
            v = self.values()
            line = self.join(v)
            pos = 0
            for i, p in enumerate(self.s.parts):
                n = len(p[1]) if p[0] == "lit" else len(v[i])
                if p[0] == "lit":
                    for cut in {pos, pos + (n + 1) // 2, pos + n}:
                        self.add(line[:cut])
                pos += n
            last = self.s.lits[-1]
            for tail in (" ", "x", " x", last, last[:1], last[-1:], "\t", '"', '" "'):
                self.add(line + tail)

    def controls(self):
        """TAB inside the [^\\s]* fields and the text fields; a few VT / FF (FALLBACK by design)"""
        for i in self.toks_of(FREE):
            for where in ("start", "mid", "end"):
                v = self.values()
                v[i] = planted(v[i], "\t", where)
                self.add(self.join(v))
        for c in ("\x0b", "\x0c"):
            for i in self.toks_of(("nospace", "lazy"))[:4]:
                v = self.values()
                v[i] = planted(v[i], c, "mid")
                self.add(self.join(v))

    # ---- the seeded part: a few mutations of a plain line each
    def mutated(self, vals, lits, kind=None):
        rng, s = self.rng, self.s
        kind = kind or rng.choice(("plant", "plant", "plant", "plant", "number", "literal", "copies", "space", "quote",
                                   "decoy", "tail"))
        if kind == "decoy":
            ds = [(g, j, a) for g in self.toks_of(("lazy", "greedy")) for j, a in self.straddles(g)]
            if ds:
                g, j, a = rng.choice(ds)
                vals[j] = vals[j] + a
            else:
                kind = "plant"
        elif kind == "tail":  # the line's last byte: one more, one less (what the tail prefilter reads)
            i = s.toks[-1]
            if s.parts[-1][0] == "lit":
                lits[-1] = rng.choice((lits[-1][:-1], lits[-1] + "x", lits[-1] + s.lits[-1][-1]))
            else:
                vals[i] = rng.choice((vals[i][:-1], vals[i] + "x", vals[i] + "-", vals[i] + " "))
        if kind == "plant":
            i = rng.choice(self.toks_of(FREE))
            vals[i] = planted(vals[i], rng.choice(s.frags), rng.choice(("start", "mid", "end", "twice")))
        elif kind == "number":
            ts = self.toks_of(NUMERIC)
            if ts:
                i = rng.choice(ts)
                edges = NUMBER_EDGES if s.parts[i][1] in ("clfnum", "num") else DECIMAL_EDGES
                vals[i] = rng.choice(edges + [vals[i] + s.next_lit(i)[:1] + "3"])
            else:  # a format without numbers: a literal of the middle loses a byte instead
                kind = "literal"
        elif kind == "copies":
            i = rng.choice(self.toks_of(FREE))
            vals[i] = planted(vals[i], s.byte * rng.choice((1, s.need - 1, s.need, s.need + 1, s.need + 5)), "mid")
        elif kind == "space":
            ts = self.toks_of(("nospace",))
            if ts:
                i = rng.choice(ts)
                vals[i] = planted(vals[i] or "x", rng.choice((" ", "\t", " y")), rng.choice(("mid", "end")))
            else:
                kind = "literal"
        elif kind == "quote":  # a '"' more or less: around the quote count of the format
            if rng.random() < 0.5 or not any('"' in l for l in lits):
                i = rng.choice(self.toks_of(FREE))
                vals[i] = planted(vals[i], '"', rng.choice(("start", "mid", "end")))
            else:
                k = rng.choice([k for k, l in enumerate(lits) if '"' in l])
                lits[k] = lits[k].replace('"', "", 1)
        if kind == "literal":  # one literal loses a byte, gets another one or is doubled
            k = rng.randrange(len(lits))
            l = lits[k]
            how = rng.randrange(3)
            lits[k] = l[1:] if how == 0 else l[:-1] + "_" if how == 1 else l + l

    def random_lines(self, n):
        target = len(self.lines) + n
        while len(self.lines) < target:
            vals = self.values()
            lits = list(self.s.lits)
            for _ in range(self.rng.choice((1, 1, 2, 2, 3))):
                self.mutated(vals, lits)
            # .* and .*? absorb whatever is planted: the more of a format's tokens they are, the more of its
            # lines get a mutation no text field can take in (else nearly every line of such a format matches)
            absorbing = len(self.toks_of(("lazy", "greedy"))) / len(self.s.toks)
            if self.rng.random() < absorbing - 0.3:
                self.mutated(vals, lits, self.rng.choice(("number", "literal", "tail")))
            self.add(self.join(vals, lits))


def build(parts, seed=SEED, n_lines=N_LINES):
    """the corpus of the format whose printed regex has these parts (regex_ref.split_regex): [bytes]"""
    b = Builder(Shape(parts), seed)
    b.plain(60)
    b.separators()
    b.need_copies()
    b.lazy_greedy()
    b.decoys(60)
    b.numbers()
    b.uplists()
    b.requests()
    b.line_ends()
    b.controls()
    if len(b.lines) > n_lines * 3 // 4:  # keep room for the seeded part: an even sample of the systematic one
        keep = n_lines * 3 // 4
        b.lines = [b.lines[k * len(b.lines) // keep] for k in range(keep)]
    b.random_lines(n_lines - len(b.lines))
    return b.lines


def short_lines(parts, seed=SEED, n=400):
    """lines of the same kind kept short (the text fields a few bytes), so that one byte chunk of the parse
    kernel holds more than 64 of them: the seeded part only"""
    b = Builder(Shape(parts), seed + 1, short=True)
    b.random_lines(n)
    return b.lines


def interleave(a, b, seed=SEED):
    """the lines of two corpora in one seeded order (a several-format handle: the routed format changes often)"""
    rng = random.Random(seed)
    out = [(0, l) for l in a] + [(1, l) for l in b]
    rng.shuffle(out)
    return out
