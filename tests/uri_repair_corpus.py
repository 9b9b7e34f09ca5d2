"""Seeded corpus of malformed URIs that HttpUriDissector repairs before
URI.create (HttpUriDissector.java:160-186), shared by test_uri_repair.py (CPU
emulation) and test_uri_repair_gpu.py.

Rules (the classes of in_scope):
  R1  bad '%' escapes (BAD_EXCAPE_PATTERN, applied twice)
  R2  "=#" -> "=", "#&" / "#?" -> "&"
  R3  several '#': all but the last become '~'
  R4  "#xHH;" not after '&' gets its '&' (ALMOST_HTML_ENCODED), then R5
  R5  unescapeHtml4: "&amp;", numeric entities that yield A-Z a-z 0-9 - _ . = &,
      and candidates the unescaper leaves alone
  MIX two or three of them in one URI
"""
import random

CLASSES = ("R1", "R2", "R3", "R4", "R5", "MIX")

# fillers: URIUtil-escaped bytes (space, {}), a second '?', a first '&' before
# any '?', '+', a valid escape, upper-case names, absolute URLs
PATHS = ["/", "/index.html", "/a/b/c.php", "/shop/item 1", "/x{y}/z", "/p%41th/", "/dir&k=v", "/~user/", "/a;b/c",
         "http://www.example.com/some/path", "https://shop.example.nl:8443/a/b", "http://10.1.2.3/"]
PARAMS = ["a=1", "b=two+words", "c=%41%42", "d=x y", "e={z}", "flag", "g=", "h=1?i=2", "Up=Case", "q=caf%C3%A9",
          "redirect=https%3A%2F%2Fwww.example.com%2Fx", "n=12341234", "k=v=w"]
FRAGS = ["", "", "top", "bla%20bla", "sec 2", "a?b&c"]

R1_TOKENS = ["%", "%%", "%%%", "%u0041", "%4", "%zz", "50%-off", "%a%a%", "%G1", "100%", "%-", "%%3d", "% 20"]
R4_TOKENS = ["#x3D;", "#x41;", "#x2D;", "#x5F;", "#x7a;", "#x2e;", "#x26;"]
R5_VALUES = ["&#x3D;", "&#61;", "&#65;", "&#x2D;", "&#X5f;", "&#46;", "&#x30;", "&#38;", "&#x26;", "&#122;"]
R5_ALONE = ["&#;", "&#x;", "&#xZZ;", "&#99999999999;", "&#12x;", "&;", "&#x1G;"]
WORDS = ["foo", "bar", "baz", "product_title", "x", "12"]


def _split(uri):
    frag = None
    if "#" in uri:
        uri, frag = uri.split("#", 1)
    query = None
    if "?" in uri:
        uri, query = uri.split("?", 1)
    return uri, query, frag


def _join(path, query, frag):
    return path + ("?" + query if query is not None else "") + ("#" + frag if frag is not None else "")


def _with_query(rng, query):
    return query if query else rng.choice(["a=1", "id=7", "s=x"])


def _at_first_sep(rng, token, query):
    # the token right after the first '?': there it meets the '&' of the "?&"
    # the reference made of that '?', and a numeric entity takes that '&' away
    return token + rng.choice(["b=1", "=1", ""]) + ("&" + query if query else "")


def _r1(rng, path, query, frag):
    t = rng.choice(R1_TOKENS)
    where = rng.randrange(4)
    if where == 0:
        path = path + t
    elif where == 1:
        query = (query + "&" if query else "") + "x=" + t + rng.choice(["", "z", "&y=2"])
    elif where == 2:
        frag = (frag or "f") + t
    elif frag is not None:
        frag = frag + t  # at the very end of the URI
    elif query is not None:
        query = query + t
    else:
        path = path + t
    return path, query, frag


def _r2(rng, path, query, frag):
    query = _with_query(rng, query)
    kind = rng.randrange(3)
    if kind == 0:
        query += "&s=#&n=" + rng.choice(WORDS)
    elif kind == 1:
        query += "#&f=" + rng.choice(WORDS)
    else:
        query += "#?f=" + rng.choice(WORDS) + "&subid=#" + rng.choice(WORDS)
    return path, query, frag


def _r3(rng, path, query, frag):
    frag = (frag or "") + "".join("#" + rng.choice(WORDS) for _ in range(rng.randint(1, 4)))
    if rng.random() < 0.3:
        frag += "#"
    return path, query, frag


def _r4(rng, path, query, frag):
    t = rng.choice(R4_TOKENS)
    r = rng.random()
    if r < 0.25:
        return path + "/seg" + t + "tail", query, frag  # ("#x26;": a '&' made before the first '?')
    if r < 0.4:
        return path, _at_first_sep(rng, t, query), frag
    query = _with_query(rng, query) + "&_r=1" + t + "12&R" + t + "E"
    return path, query, frag


def _r5(rng, path, query, frag):
    if rng.random() < 0.15:
        return path, _at_first_sep(rng, rng.choice(R5_VALUES + ["&amp;"])[1:], query), frag
    query = _with_query(rng, query)
    kind = rng.randrange(4)
    if kind == 0:
        query = query.replace("&", "&amp;") + "&amp;last=1"
    elif kind == 1:
        query += "&sort" + rng.choice(R5_VALUES[:2]) + "price&v=" + rng.choice(R5_VALUES) + rng.choice(R5_VALUES)
    elif kind == 2:
        query += "&w=" + rng.choice(R5_ALONE) + "1&t=2"
    else:
        query += "?amp;o=1&amp;amp;p=" + rng.choice(R5_VALUES)
    return path, query, frag


_PLANT = {"R1": _r1, "R2": _r2, "R3": _r3, "R4": _r4, "R5": _r5}


def plant(rng, uri, cls):
    """uri with one defect of class cls (MIX: two or three classes) planted."""
    path, query, frag = _split(uri)
    kinds = rng.sample(sorted(_PLANT), rng.randint(2, 3)) if cls == "MIX" else [cls]
    for k in kinds:
        path, query, frag = _PLANT[k](rng, path, query, frag)
    return _join(path, query, frag)


def clean_uri(rng, absolute=False):
    path = rng.choice([p for p in PATHS if p.startswith("http")] if absolute else PATHS)
    query = "&".join(rng.sample(PARAMS, rng.randint(0, 4))) or None
    frag = rng.choice(FRAGS) or None
    if query and frag and query.endswith("="):
        query += "0"  # ("=#" is a defect of class R2)
    return _join(path, query, frag)


def line(rng, k, uri, referer):
    return ('10.%d.%d.%d - - [%02d/Oct/2026:13:%02d:%02d +0200] "GET %s HTTP/1.1" %d %d "%s" "Mozilla/5.0 (X11) k%d"'
            % (rng.randrange(256), rng.randrange(256), rng.randrange(1, 255), 1 + k % 28, k % 60, rng.randrange(60), uri,
               rng.choice([200, 200, 304, 404]), rng.randrange(100000), referer, k)).encode("ascii")


def in_scope_line(rng, k, cls=None, referer=None):
    """One `combined` line whose request URI carries a defect of class cls
    (default: the k-th class in turn), and whose referer does on half of them."""
    cls = cls or CLASSES[k % len(CLASSES)]
    uri = plant(rng, clean_uri(rng), cls)
    if referer is None:
        referer = clean_uri(rng, absolute=True) if rng.random() < 0.8 else "-"
        if rng.random() < 0.5:
            referer = plant(rng, clean_uri(rng, absolute=True), rng.choice(CLASSES))
    return line(rng, k, uri, referer)


def clean_line(rng, k):
    return line(rng, k, clean_uri(rng), clean_uri(rng, absolute=True))


def in_scope(seed, n):
    """n `combined` lines, every request URI defective (the classes in turn:
    each has at least n / 8 lines), half of the referers too."""
    rng = random.Random(seed)
    return [in_scope_line(rng, k) for k in range(n)]


def clean(seed, n):
    rng = random.Random(seed)
    return [clean_line(rng, k) for k in range(n)]


def out_of_scope():
    """Request URIs that stay FALLBACK: named entities outside amp / lt / gt /
    quot, numeric entities >= 0x80, non-ASCII bytes."""
    rng = random.Random(0)
    uris = ["/a?x=&eacute;", "/a?x=1&hearts;y=2", "/a?x=&nosuch;", "/a?x=&#233;", "/ünï?x=%zz"]
    return [line(rng, k, u, "-") if u.isascii() else
            ('1.2.3.4 - - [01/Oct/2026:13:00:00 +0200] "GET %s HTTP/1.1" 200 1 "-" "ua"' % u).encode("utf-8")
            for k, u in enumerate(uris)]
