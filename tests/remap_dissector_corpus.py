"""The corpus of the remapped-value dissector tests (ScreenResolutionDissector,
ModUniqueIdDissector): 1,000 'combined'-shaped lines with a "%{UNIQUE_ID}e"
"%{X-Res}i" tail, whose request carries s= and uid= parameters.  1,000 is no
multiple of 64 (the last wave is partial), and the categories cycle with
periods 16 / 17 (screen values: parameter / token) and 19 / 13 (unique ids:
parameter / token), all pairwise coprime, so that neighbouring lanes diverge and
every pair of categories meets.  Everything is ASCII with valid escapes only.

Each line comes with the source values it planted, DECODED as the dissectors see
them (None: no value -- the parameter absent, the token "-"), and whether a
parameter repeats; the expectations are remap_dissector_ref's rules applied to
those values.  `throws` is the generator's own statement of which planted screen
values make the reference throw when width and height are both requested."""
import base64
import random

import remap_dissector_ref as ref

LOGFORMAT = '%h %l %u %t "%r" %>s %b "%{Referer}i" "%{User-Agent}i" "%{UNIQUE_ID}e" "%{X-Res}i"'
Q = "request.firstline.uri.query."
P_S, P_UID = Q + "s", Q + "uid"
T_UID, T_RES = "server.environment.unique_id", "request.header.x-res"
REMAPS = [(P_S, "SCREENRESOLUTION"), (P_UID, "MOD_UNIQUE_ID"), (T_UID, "MOD_UNIQUE_ID"), (T_RES, "SCREENRESOLUTION")]
DISSECTORS = [("ScreenResolutionDissector", "x")]
# handle A: today's program -- the same format, remaps and these fields
FIELDS_A = ["IP:connection.client.host", "TIME.EPOCH:request.receive.time.epoch", "HTTP.URI:request.firstline.uri",
            "STRING:" + P_S, "STRING:" + P_UID, "VARIABLE:" + T_UID, "HTTP.HEADER:" + T_RES,
            "STRING:request.status.last", "HTTP.USERAGENT:request.user-agent"]
SCREEN_OUT = [("SCREENWIDTH", "width"), ("SCREENHEIGHT", "height")]
UID_OUT = [("TIME.EPOCH", "epoch"), ("IP", "ip"), ("PROCESSID", "processid"), ("COUNTER", "counter"),
           ("THREAD_INDEX", "threadindex")]
# handle B adds the new outputs (in the reference's delivery order per source)
NEW_FIELDS = (["%s:%s.%s" % (t, P_S, n) for t, n in SCREEN_OUT] + ["%s:%s.%s" % (t, P_UID, n) for t, n in UID_OUT] +
              ["%s:%s.%s" % (t, T_UID, n) for t, n in UID_OUT] + ["%s:%s.%s" % (t, T_RES, n) for t, n in SCREEN_OUT])
FIELDS_B = FIELDS_A + NEW_FIELDS

ABSENT, TWICE = "absent", "twice"
# (raw text in the line, the decoded value, throws with width and height requested)
SCREEN_PARAM = [
    ("1280x800", "1280x800", False), ("1024x768x32", "1024x768x32", False), ("x800", "x800", False),
    ("1280x", "1280x", True), ("x", "x", True), ("xx", "xx", True), ("1280", "1280", False), ("", "", False),
    ("1280X800", "1280X800", False), ("1280%78800", "1280x800", False), ("1280x+800", "1280x 800", False),
    ("+5x-3", " 5x-3", False), ("%2B5x-3", "+5x-3", False), ("9223372036854775808x1", "9223372036854775808x1", False),
    (ABSENT, None, False), (TWICE, None, False),
]
# the token is not URL-decoded: its '+' and '%78' stay
SCREEN_TOKEN = [
    ("1280x800", False), ("1024x768x32", False), ("x800", False), ("1280x", True), ("x", True), ("xx", True),
    ("1280", False), ("", False), ("1280X800", False), ("1280%78800", False), ("1280x+800", False), ("+5x-3", False),
    ("9223372036854775808x1", False), ("-", False), ("1x2x", False), ("3840x2160", False), ("xx7", False),
]
REFERENCE_IDS = ["VaGTKApid0AAALpaNo0AAAAC", "Ucdv38CoEJwAAEusp6EAAADz"]  # TestModUniqueIdDissector.java:37,58


def _random_id(rng, urlsafe):
    """the id of 18 random bytes: letters and digits only, or with '-' / '_' in it"""
    while True:
        t = base64.urlsafe_b64encode(bytes(rng.randrange(256) for _ in range(18))).decode()
        if (("-" in t or "_" in t) and "+" not in t) == urlsafe:
            return t


def _id_values(rng, k):
    """the k-th unique-id text of a source (k counts that source's lines)"""
    good = REFERENCE_IDS[0]
    kinds = [
        lambda: _random_id(rng, False), lambda: _random_id(rng, True), lambda: REFERENCE_IDS[0],
        lambda: REFERENCE_IDS[1], lambda: good[:7] + "@" + good[8:], lambda: good[:11] + "+" + good[12:],
        lambda: good[:3] + "/" + good[4:], lambda: good[:20] + "=" + good[21:], lambda: good[:23] + "!",
        lambda: "", lambda: REFERENCE_IDS[1][:23], lambda: REFERENCE_IDS[1] + "A", lambda: _random_id(rng, True),
    ]
    return kinds[k % len(kinds)]()


def corpus(n=1000, seed=20261021):
    """(data bytes, lines): per line a dict with the planted values (s, uid:
    the parameters; tuid, tres: the tokens; decoded, None = no value), s_twice /
    uid_twice, and throws (a planted screen value that throws)."""
    rng = random.Random(seed)
    out, lines = [], []
    for i in range(n):
        raw_s, s_val, s_thr = SCREEN_PARAM[i % 16]
        tres_raw, t_thr = SCREEN_TOKEN[i % 17]
        uk = i % 19  # the parameter: 13 texts, then absent / twice, and the '+' id four more times
        if uk < 13:
            uid_raw = _id_values(rng, uk)
        elif uk == 13:
            uid_raw = ABSENT
        elif uk == 14:
            uid_raw = TWICE
        else:
            uid_raw = _id_values(rng, 5 if uk % 2 else 0)
        tk = i % 13
        tuid_raw = "-" if tk == 12 else _id_values(rng, tk if tk != 9 else 12)  # (an empty token: covered by X-Res)
        q = ["a=%d" % i]
        if raw_s == TWICE:
            q += ["s=1280x800", "b=2", "s=1024x768"]
        elif raw_s != ABSENT:
            q.append("s=" + raw_s)
        if uid_raw == TWICE:
            q += ["uid=" + REFERENCE_IDS[0], "uid=" + REFERENCE_IDS[1]]
        elif uid_raw != ABSENT:
            q.append("uid=" + uid_raw)
        q.append("z=%d" % (i % 7))
        line = ('10.%d.%d.%d - - [05/Sep/2010:11:%02d:%02d +0200] "GET /p/%d?%s HTTP/1.1" 200 %d "-" "agent/%d" "%s" "%s"'
                % (i % 250, (i // 3) % 250, i % 199, i % 60, (i * 7) % 60, i, "&".join(q), 100 + i, i % 5, tuid_raw,
                   tres_raw))
        assert all(32 <= ord(ch) < 127 for ch in line)
        out.append(line)
        lines.append({
            "s": s_val, "s_twice": raw_s == TWICE,
            "uid": None if uid_raw in (ABSENT, TWICE) else uid_raw.replace("+", " "), "uid_twice": uid_raw == TWICE,
            "tuid": None if tuid_raw == "-" else tuid_raw, "tres": None if tres_raw == "-" else tres_raw,
            "throws": (s_thr and raw_s not in (ABSENT, TWICE)) or t_thr,
        })
    return ("\n".join(out) + "\n").encode("ascii"), lines


def expected(ln, want_w=True, want_h=True, want_uid=True):
    """the new outputs of one line: {"TYPE:path": str | int}, or None where the
    line is FALLBACK (a repeated parameter below which an output is requested,
    or the reference throws)"""
    if ln["s_twice"] or (ln["uid_twice"] and want_uid):
        return None
    exp = {}
    try:
        for path, v in ((P_S, ln["s"]), (T_RES, ln["tres"])):
            got = ref.screen(v, want_w, want_h)
            for t, n in SCREEN_OUT:
                if n in got:
                    exp["%s:%s.%s" % (t, path, n)] = got[n]
    except IndexError:
        return None
    for path, v in ((P_UID, ln["uid"]), (T_UID, ln["tuid"])):
        got = ref.unique_id(v) if want_uid else {}
        for t, n in UID_OUT:
            if n in got:
                exp["%s:%s.%s" % (t, path, n)] = got[n]
    return exp


# ---- a program without URI, list or cookie stages: only the X-Res token's outputs and the client host are
# requested, so nothing but the value stage's guard runs after the parse kernels
TOKEN_ONLY_FIELDS = ["IP:connection.client.host"] + ["%s:%s.%s" % (t, T_RES, n) for t, n in SCREEN_OUT]
TOKEN_ONLY_REMAPS = [(T_RES, "SCREENRESOLUTION")]


def expected_token_only(ln, want_w=True, want_h=True):
    """the X-Res token's outputs of one line, None where the reference throws"""
    try:
        got = ref.screen(ln["tres"], want_w, want_h)
    except IndexError:
        return None
    return {"%s:%s.%s" % (t, T_RES, n): got[n] for t, n in SCREEN_OUT if n in got}


def planted_fallbacks(lines):
    """the generator's own count of the lines it planted a FALLBACK cause in"""
    return sum(1 for ln in lines if ln["s_twice"] or ln["uid_twice"] or ln["throws"])


def as_string(v):
    """the STRING column of a value: Long.toString of a long"""
    return str(v) if isinstance(v, int) else v


def as_long(v):
    """the LONG column of a value: the long, or Value.getLong of the string (None: null)"""
    return v if isinstance(v, int) else ref.java_parse_long(v)


# ---- a nested source: a parameter of a derived URI's query (request.firstline.uri.query.g remapped to
# HTTP.URI, its query's s remapped to SCREENRESOLUTION), 64 lines
G_S = Q + "g.query.s"
NESTED_REMAPS = [(Q + "g", "HTTP.URI"), (G_S, "SCREENRESOLUTION")]
NESTED_FIELDS = ["STRING:" + Q + "g", "SCREENWIDTH:%s.width" % G_S, "SCREENHEIGHT:%s.height" % G_S]
# (the text inside g's URL before g is escaped, the decoded value, FALLBACK)
NESTED_S = [("s=1280x800", "1280x800", False), ("s=x800", "x800", False), ("s=1280x", "1280x", True),
            ("s=1280%78800", "1280x800", False), ("k=1", None, False), ("s=1x2&s=3x4", None, True),
            ("s=1024x768x32", "1024x768x32", False), ("s=x", "x", True), ("s=1280", "1280", False),
            ("s=7x+8", "7x 8", False), (None, None, False)]


def nested_corpus(n=64):
    """(data bytes, per line the expected new outputs or None for FALLBACK)"""
    out, exp = [], []
    for i in range(n):
        inner, val, fb = NESTED_S[i % len(NESTED_S)]
        q = ["a=%d" % i]
        if inner is not None:
            url = "http://h%d.example/p?%s&t=%d" % (i % 3, inner, i)
            q.append("g=" + "".join(ch if ch.isalnum() or ch in ".-_" else "%%%02X" % ord(ch) for ch in url))
        out.append('10.0.0.%d - - [05/Sep/2010:11:27:%02d +0200] "GET /n/%d?%s HTTP/1.1" 200 %d "-" "agent" "-" "-"'
                   % (i, i % 60, i, "&".join(q), i))
        if fb:
            exp.append(None)
            continue
        got = ref.screen(val, True, True)
        exp.append({"%s:%s.%s" % (t, G_S, nm): got[nm] for t, nm in SCREEN_OUT if nm in got})
    return ("\n".join(out) + "\n").encode("ascii"), exp
