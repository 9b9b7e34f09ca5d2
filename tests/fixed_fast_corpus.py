"""Lines for the straight-line first leaf of the fixed-shape instances
(lp_device.h fixed_fast_leaf): every position the walk takes from the plane
words on the edges of those words and of its limits, and every check it makes
on the bytes failing one at a time.  Shared by the CPU tests
(test_fixed_fast.py, which re-derives the edge cases from the bytes) and the
GPU test.  Lines are bytes without terminator, (name, line) pairs."""

HEAD = 128   # bytes of the head words (ff::HEAD_WORDS)
TAIL = 384   # bytes of the tail words (ff::TAIL_WORDS)
DIGITS = 12  # digits of a CLFNUMBER the SWAR test covers (ff::NUM_BYTES)
STATUS = 64  # bytes from the start of %>s in which its closing ' ' must lie (ff::STATUS_BYTES)
MAX_LINE = 8191
EDGE_BITS = (0, 31, 32, 63)

T0 = b"10/Oct/2026:13:55:36 -0700"
F = dict(h=b"203.0.113.7", l=b"-", u=b"frank", t=T0, r=b"GET /a.gif?x=1&y=2 HTTP/1.1", s=b"200", b=b"2326",
         ref=b"http://www.example.com/start.html?q=x", ua=b"Mozilla/5.0 (X11; Linux x86_64) Firefox/115.0")
# the separators of "combined", by name, in order
SEPS = (("hl", b" "), ("lu", b" "), ("ut", b" ["), ("tr", b'] "'), ("rs", b'" '), ("sb", b" "), ("bref", b' "'),
        ("refua", b'" "'), ("end", b'"'))


def combined(sep=None, **kw):
    f = dict(F, **kw)
    s = dict(SEPS, **(sep or {}))
    return (f["h"] + s["hl"] + f["l"] + s["lu"] + f["u"] + s["ut"] + f["t"] + s["tr"] + f["r"] + s["rs"] + f["s"] +
            s["sb"] + f["b"] + s["bref"] + f["ref"] + s["refua"] + f["ua"] + s["end"])


def common(sep=None, **kw):
    f = dict(F, **kw)
    s = dict(SEPS, **(sep or {}))
    return (f["h"] + s["hl"] + f["l"] + s["lu"] + f["u"] + s["ut"] + f["t"] + s["tr"] + f["r"] + s["rs"] + f["s"] +
            s["sb"] + f["b"])


def pad(n, c=b"a"):
    return c * max(0, n)


def fixed_len(make, field, total, **kw):
    """make(...) with `field` padded so that the line is `total` bytes long"""
    base = len(make(**dict(kw, **{field: b""})))
    return make(**dict(kw, **{field: pad(total - base)}))


def _shared(make, name, tail_fields):
    """the cases both shapes have; tail_fields: the padded field that moves the
    quote that closes %r away from the end of the line"""
    out = []
    add = lambda n, l: out.append(("%s/%s" % (name, n), l))
    add("valid", make())
    # ---- head words: the three separators on the edge bits of both words, and the head limit
    for w in range(2):
        for bit in EDGE_BITS:
            pos = 64 * w + bit
            add("s1@%d" % pos, make(h=pad(pos)))                      # (pos 0: an empty %h)
            if pos >= 2:
                add("s2@%d" % pos, make(h=b"", l=pad(pos - 1, b"7")))      # (a long %l: the digit test's limit too)
                add("s2@%d/short-l" % pos, make(h=pad(pos - 2), l=b"-"))
            if pos >= 4:
                add("s3@%d" % pos, make(h=b"h", l=b"-", u=pad(pos - 4)))
    for pos in (HEAD - 2, HEAD - 1, HEAD, HEAD + 1):
        add("s3@%d/long-h" % pos, make(h=pad(pos - 8), l=b"-", u=b"frank"))
        add("s3@%d/long-u" % pos, make(h=b"h", l=b"-", u=pad(pos - 4)))
    # ---- lines around the limits' lengths and MAX_LINE
    short = dict(h=b"h", u=b"u", r=b"GET / HTTP/1.1", ref=b"-", ua=b"-")  # (the valid line is longer than the head)
    for total in (HEAD - 1, HEAD, HEAD + 1, TAIL - 1, TAIL, TAIL + 1, 511, 512, 513):
        add("len%d" % total, fixed_len(make, tail_fields, total, **{k: v for k, v in short.items() if k != tail_fields}))
        add("len%d/long-r" % total, fixed_len(make, "r", total, **{k: v for k, v in short.items() if k != "r"}))
    for total in (MAX_LINE - 1, MAX_LINE, MAX_LINE + 1):
        add("len%d" % total, fixed_len(make, tail_fields, total))
        add("len%d/long-r" % total, fixed_len(make, "r", total))
    # ---- whitespace at separators: TAB for each space, doubled spaces
    for key, lit in SEPS:
        if make is common and key in ("bref", "refua", "end"):  # (separators a common line does not have)
            continue
        for k in range(len(lit)):
            if lit[k:k + 1] == b" ":
                add("tab/%s" % key, make(sep={key: lit[:k] + b"\t" + lit[k + 1:]}))
                add("double-space/%s" % key, make(sep={key: lit[:k] + b"  " + lit[k + 1:]}))
            add("drop/%s/%d" % (key, k), make(sep={key: lit[:k] + lit[k + 1:]}))
            add("other/%s/%d" % (key, k), make(sep={key: lit[:k] + b"X" + lit[k + 1:]}))
    # ---- token shapes: empty and "-" tokens, numbers
    for fld in ("h", "l", "u", "r", "s", "b", "ref", "ua"):
        add("empty/%s" % fld, make(**{fld: b""}))
        add("dash/%s" % fld, make(**{fld: b"-"}))
        add("zero/%s" % fld, make(**{fld: b"0"}))
        add("space-in/%s" % fld, make(**{fld: b"a b"}))
        add("tab-in/%s" % fld, make(**{fld: b"a\tb"}))
        add("quote-in/%s" % fld, make(**{fld: b'a"b'}))
        add("quote-space-in/%s" % fld, make(**{fld: b'a" b'}))
    for fld in ("l", "b"):
        for v in (b"7", b"12x", b"x12", b"1-", b"--", b"-1", b"1" * (DIGITS - 1), b"1" * DIGITS, b"1" * (DIGITS + 1),
                  b"1" * 40, b"1" * (DIGITS - 1) + b"x", b"1" * DIGITS + b"x"):
            add("num/%s/%s" % (fld, v[:16].decode()), make(**{fld: v}))
    for v in (b"2", b"20", b"2000", b"abc", b"20x", b'2"0'):
        add("status/%s" % v.decode(), make(s=v))
    for k in (STATUS - 2, STATUS - 1, STATUS, STATUS + 1):
        add("status-len/%d" % k, make(s=pad(k, b"2")))
    # ---- request-line shapes (the first-line stage runs on the spans of either path)
    for r in (b"GET /x HTTP/1.1", b"GET /x HTTP/10.0", b"GET /x HTTP/1.10", b"GET /x http/1.1", b"GET /x", b"GET",
              b"GET ", b"GET /x HTTP/1.", b"GET /x  HTTP/1.1", b"GET /x\tHTTP/1.1", b"GET\t/x HTTP/1.1",
              b"M-SEARCH /x HTTP/1.1", b"VERSION_CONTROL /x HTTP/1.1", b"BASELINE-CONTROL /x HTTP/1.1",
              b"PROPFIND9 /x HTTP/1.1", b"G3T /x HTTP/1.1", b"get /x y z HTTP/1.1", b"/x HTTP/1.1", b" /x HTTP/1.1",
              b'GET /x?q="a" HTTP/1.1', b'GET /x" HTTP/1.1', b'GET /x" y HTTP/1.1'):
        add("request/%s" % r.decode().replace("\t", "\\t"), make(r=r))
    # ---- time stamps
    for t in (b"10/Foo/2026:13:55:36 -0700", b"10/Oct/2026:24:55:36 -0700", b"10/Oct/2026:13:55:36 |0700",
              b"10/Oct/2026:13:55:36 +0700", b"40/Oct/2026:13:55:36 -0700", b"10/Oct/0026:13:55:36 -0700",
              b"10/Oct/2026:13:55:36 -070", b"10/Oct/2026:13:55:36  0700", b"10/Oct/2026 13:55:36 -0700",
              b"1/Oct/2026:13:55:36 -0700", b"10/Oct/2026:13:55:36 -07000", T0 + b"]", b"[" + T0):
        add("time/%s" % t.decode(), make(t=t))
    # ---- line ends: '\r' left on, bytes after the last token
    for tail in (b"\r", b" ", b"\t", b"x", b'"', b' "', b' "x"', b' "-" "-"', b" -", b"7"):
        add("tail/%r" % tail, make() + tail)
    v = make()
    for cut in (1, 2, 3, 5, 20, len(v) - 40, len(v) - 1):
        add("cut/%d" % cut, v[:len(v) - cut])
    for fld in ("h", "u", "r", "ref", "ua"):
        add("utf8/%s" % fld, make(**{fld: "café".encode()}))
        add("del/%s" % fld, make(**{fld: b"a\x7fb"}))
    return out


def combined_cases():
    out = _shared(combined, "combined", "ua")
    add = lambda n, l: out.append(("combined/%s" % n, l))
    # ---- tail words: Q2 (d bytes before the end: the user agent is d - 2 long) and Q5 on the edge
    # bits of every word, and Q5 around the tail limit.  After Q5 come ` 200 7 "` (8), the referer,
    # `" "` (3), the user agent and `"`: Q5 is 13 + len(ref) + len(ua) bytes before the end.
    for w in range(TAIL // 64):
        for bit in EDGE_BITS:
            d = TAIL - (64 * w + bit)  # the quote is bit `bit` of tail word w when it lies d bytes before the end
            if d >= 2:
                add("Q2@w%d.%d" % (w, bit), combined(ua=pad(d - 2)))
            if d >= 13:
                add("Q5@w%d.%d/long-ua" % (w, bit), combined(s=b"200", b=b"7", ref=b"", ua=pad(d - 13)))
                add("Q5@w%d.%d/long-ref" % (w, bit), combined(s=b"200", b=b"7", ref=pad(d - 13), ua=b""))
    for d in (TAIL - 2, TAIL - 1, TAIL, TAIL + 1, TAIL + 2, TAIL + 64):
        add("Q5-%d/long-ua" % d, combined(s=b"200", b=b"7", ref=b"r", ua=pad(d - 14)))
        add("Q5-%d/long-ref" % d, combined(s=b"200", b=b"7", ref=pad(d - 14), ua=b"u"))
    # ---- quote counts after the request's start (a valid line has 5) and their placement
    add("quotes4", combined(sep={"refua": b" "}))
    add("quotes4/no-end", combined(sep={"end": b""}))
    add("quotes3", combined(sep={"refua": b" ", "end": b""}))
    add("quotes6/r", combined(r=b'GET /x?a="1 HTTP/1.1'))
    add("quotes7/r", combined(r=b'GET /x?a="1" HTTP/1.1'))
    add("quotes7/r-lit", combined(r=b'GET /x" 200 7 "y HTTP/1.1'))
    add("quotes6/ref", combined(ref=b'http://a/"b'))
    add("quotes7/ref-lit", combined(ref=b'http://a/" "b'))
    add("quotes6/ua", combined(ua=b'Moz"illa'))
    add("quotes7/ua-lit", combined(ua=b'Moz" "illa'))
    add("quotes/ua-ends-quote", combined(ua=b'Mozilla"'))
    add("quotes/h", combined(h=b'1.2"3.4'))
    add("quotes/u", combined(u=b'fr"ank'))
    add("quotes/h-lit", combined(h=b'1.2"'))
    add("Q3+2!=Q2/x", combined(sep={"refua": b'" x"'}))
    add("Q3+2!=Q2/2sp", combined(sep={"refua": b'"  "'}))
    add("Q3+2!=Q2/none", combined(sep={"refua": b'""'}))
    add("Q3+1/tab", combined(sep={"refua": b'"\t"'}))
    add("common-line", common())
    return out


def common_cases():
    out = _shared(common, "common", "r")
    add = lambda n, l: out.append(("common/%s" % n, l))
    # the last quote d bytes before the end (`" 200 ` then %b: d = 6 + len(b)), on the tail words' edge bits
    for w in range(TAIL // 64):
        for bit in EDGE_BITS:
            d = TAIL - (64 * w + bit)
            if d >= 7:
                add("QL@w%d.%d/long-s" % (w, bit), common(s=pad(d - 4, b"2"), b=b"7"))
            if 7 <= d <= 6 + DIGITS + 2:
                add("QL@w%d.%d/long-b" % (w, bit), common(b=pad(d - 6, b"7")))
    for d in (TAIL - 1, TAIL, TAIL + 1, TAIL + 2):
        add("QL-%d" % d, common(s=pad(d - 4, b"2"), b=b"7"))
    add("quotes2/r", common(r=b'GET /x?a="1 HTTP/1.1'))
    add("quotes/r-lit", common(r=b'GET /x" 200 7 HTTP/1.1'))
    add("quotes/after", common(b=b'7"'))
    add("quotes/after-lit", common(b=b'7" 200 7'))
    add("no-quote", common(sep={"rs": b" "}))
    add("combined-line", combined())
    return out


def cases(shape):
    return combined_cases() if shape == "combined" else common_cases()


def lines(shape):
    return [l for _, l in cases(shape)]
