"""An independent reference for the LogFormat matcher: Python's `re`.

Every other test of csrc/lp_device.h's match_line compares it with oracle/,
whose jregex.c is this project's own restatement of java.util.regex.  Python's
`re` is a leftmost-first backtracking matcher written by other people: the
regex that TokenFormatDissector builds (Oracle.regex()) is translated
mechanically (java_to_py) and run by `re`; the group texts are what the
dissector hands on (decodeExtractedValue: "-" becomes null, every other text
as it is).

Test infrastructure only.  Shared by test_regex_priority.py (oracle and CPU
emulation against `re`) and test_regex_priority_gpu.py (the kernels against
`re`); the lines are regex_corpus.py's.
"""
import re

# ---------------------------------------------------------------- the formats
COMBINED = ["IP:connection.client.host", "NUMBER:connection.client.logname", "STRING:connection.client.user",
            "TIME.STAMP:request.receive.time", "HTTP.FIRSTLINE:request.firstline", "STRING:request.status.last",
            "BYTESCLF:response.body.bytes", "HTTP.URI:request.referer", "HTTP.USERAGENT:request.user-agent"]
_USER, _HOST, _FIRST, _STATUS, _BYTES = COMBINED[2], COMBINED[0], COMBINED[4], COMBINED[5], COMBINED[6]
_TIME, _REF, _UA = COMBINED[3], COMBINED[7], COMBINED[8]

# name -> (LogFormat, GROUPS: per capture group the token-level output path that carries its text)
FORMATS = {
    # the Apache family of the fixed-shape kernel instances
    "combined": ("combined", COMBINED),
    "common": ("common", COMBINED[:7]),
    # three lazy fields in a row
    "cookie": ('%h %l %u %t "%r" %>s %b "%{Referer}i" "%{User-Agent}i" "%{Cookie}i"',
               COMBINED + ["HTTP.COOKIES:request.cookies"]),
    # separators longer than 4 bytes: the long-literal path of lit_at / lit_first / lit_last
    # (the number in the middle gives the greedy .* candidates that fail: '%{User-Agent}i -- sep -- %r -- sep -- %>s'
    # has none, every match of it is the first leaf)
    "longlit": ("%{User-Agent}i -- sep -- %r -- sep -- %b -- sep -- %{Referer}i -- sep -- %D",
                [_UA, _FIRST, _BYTES, _REF, "MICROSECONDS:response.server.processing.time"]),
    # no spaces between tokens: a number directly against a quote, a non-det [^\s]* followed by '"'
    "nospace": ('%u %h "%r"%>s%b"%{Referer}i""%{User-Agent}i"', [_USER, _HOST, _FIRST, _STATUS, _BYTES, _REF, _UA]),
    # the greedy .* followed by '] [' with need > 1
    "brackets": ("[%t] [%r] [%{Referer}i] [%{User-Agent}i]", [_TIME, _FIRST, _REF, _UA]),
    # the last element .* / [^\s]* (e.last), after a lazy field whose first candidates can fail at the number
    "end_greedy": ('%h "%{Referer}i" %b %r', [_HOST, _REF, _BYTES, _FIRST]),
    "end_nospace": ('%t "%{Referer}i" %b %>s', [_TIME, _REF, _BYTES, _STATUS]),
    # NGINX: the literal-aware instance, EK_NOSPACE3, the upstream lists, EK_MSEC, EK_TIME_ISO; its first token is
    # not an IP (FORMAT_IP's nested {0,8} is exponential in a backtracking engine; test_ipv6_hosts.py owns it)
    "nginx": ('$remote_user [$time_iso8601] $msec "$request" $status $upstream_response_time $upstream_addr '
              '"$http_user_agent"',
              [_USER, "TIME.ISO8601:request.receive.time", "TIME.EPOCH_SECOND_MILLIS:request.receive.time.epoch",
               _FIRST, _STATUS, "UPSTREAM_SECOND_MILLIS_LIST:nginxmodule.upstream.response.time",
               "UPSTREAM_ADDR_LIST:nginxmodule.upstream.addr", _UA]),
    # NGINX tokens tight against each other and against literals their own text can hold: a fraction directly
    # followed by a number and a number by [0-9]+|- (EK_DECIMAL's shorter fraction, a shorter digit run), "$request" and
    # [^\s]* followed by '"' (the literal-aware first candidates, the shorter third run), an upstream list
    # followed by ', ' (uplist_prev_end: fewer items)
    "nginx_tight": ('$request_time$body_bytes_sent"$request"$status"$http_user_agent" $upstream_response_time, '
                    '$hostname $pid$connection_requests',
                    ["SECOND_MILLIS:response.server.processing.time", "BYTES:response.body.bytes",
                     _FIRST, _STATUS, _UA,
                     "UPSTREAM_SECOND_MILLIS_LIST:nginxmodule.upstream.response.time", "STRING:connection.client.host",
                     "NUMBER:connection.server.child.processid", "NUMBER:connection.requestnr"]),
}
# several formats in one handle: (the handle's name, its formats in order); no line of its corpus matches both
MULTI = {"nospace+brackets": ("nospace", "brackets")}


def logformat(name):
    if name in MULTI:
        return "\n".join(FORMATS[f][0] for f in MULTI[name])
    return FORMATS[name][0]


def fields(name):
    """the paths to request: exactly the groups' (a several-format handle: of all its formats)"""
    out = []
    for f in MULTI.get(name, (name,)):
        out += [p for p in FORMATS[f][1] if p not in out]
    return out


# ---------------------------------------------------------------- Java -> Python
class Untranslatable(ValueError):
    """a construct java_to_py does not know, or one that Java and Python read differently"""


# java.util.regex without flags: '.' matches any character but a line terminator, '$' the end of the input or the
# place before a final line terminator.  Python's read only '\n' as one, so both are spelled out.
_LINE_TERMS = "\\n\\r\\x85\\u2028\\u2029"
_DOT = "[^" + _LINE_TERMS + "]"
_DOLLAR = "(?=(?:\\r\\n|[" + _LINE_TERMS + "])?\\Z)"
_ESCAPES = set("s") | set(".+-\\|[](){}*?^$/:\"'")  # \s is [ \t\n\x0B\f\r] in Java and, with re.ASCII, in Python


def _escape(rx, i, where):
    if i + 1 >= len(rx) or rx[i + 1] not in _ESCAPES:
        raise Untranslatable("escape %r %s at %d" % (rx[i:i + 2], where, i))
    return rx[i:i + 2]


def java_to_py(rx):
    """The java.util.regex pattern rx as a Python `re` pattern (compile it as str with re.ASCII).  Knows what the
    token tables use: \\Q..\\E, groups, (?:..), classes, the greedy and lazy quantifiers, {m,n}, |, ^, $, '.'.
    Raises Untranslatable on anything else (possessive quantifiers, \\p{..}, \\h, \\d, back references, flags,
    look-around, class unions and intersections, ...) instead of passing it through."""
    out = []
    i, n = 0, len(rx)
    quantified = 0  # the previous item was a quantifier (1; a '+' after it would be possessive) or its lazy mark (2)
    while i < n:
        c = rx[i]
        was_quantified, quantified = quantified, 0
        if rx.startswith("\\Q", i):
            j = rx.find("\\E", i + 2)
            if j < 0:
                raise Untranslatable("\\Q without \\E at %d" % i)
            out.append(re.escape(rx[i + 2:j]))
            i = j + 2
        elif c == "\\":
            out.append(_escape(rx, i, "outside a class"))
            i += 2
        elif c == "[":
            j = i + 1
            cls = ["["]
            if j < n and rx[j] == "^":
                cls.append("^")
                j += 1
            first = True
            while j < n and (rx[j] != "]" or first):
                if rx[j] == "\\":
                    cls.append(_escape(rx, j, "in a class"))
                    j += 2
                elif rx[j] == "[" or rx.startswith("&&", j):
                    raise Untranslatable("class union / intersection at %d" % j)
                elif rx[j] == "]":
                    raise Untranslatable("']' first in a class at %d" % j)
                else:
                    cls.append(rx[j])
                    j += 1
                first = False
            if j >= n:
                raise Untranslatable("unterminated class at %d" % i)
            out.append("".join(cls) + "]")
            i = j + 1
        elif c == "(":
            if rx.startswith("(?", i):
                if not rx.startswith("(?:", i):
                    raise Untranslatable("group construct %r at %d" % (rx[i:i + 4], i))
                out.append("(?:")
                i += 3
            else:
                out.append("(")
                i += 1
        elif c in "*+?" or c == "{":
            if was_quantified == 1 and c == "+":
                raise Untranslatable("possessive quantifier at %d" % i)
            if was_quantified == 2 or (was_quantified == 1 and c != "?"):
                raise Untranslatable("quantifier after a quantifier at %d" % i)
            if not out or out[-1] in ("(", "(?:", "|", "^"):
                raise Untranslatable("quantifier with nothing before it at %d" % i)
            if c == "{":
                m = re.compile(r"\{[0-9]+(?:,[0-9]*)?\}").match(rx, i)
                if not m:
                    raise Untranslatable("'{' that is no {m,n} at %d" % i)
                out.append(m.group())
                i = m.end()
            else:
                out.append(c)
                i += 1
            quantified = 2 if was_quantified else 1  # 2: the lazy mark, nothing may follow it
        elif c == ".":
            out.append(_DOT)
            i += 1
        elif c == "$":
            out.append(_DOLLAR)
            i += 1
        elif c in ")|^" or c.isalnum() or c in " /:,-\"'%_=<>@!~;&#":
            out.append("\\" + c if c == "#" else c)
            i += 1
        else:
            raise Untranslatable("character %r at %d" % (c, i))
    return "".join(out)


def split_regex(rx):
    """the regex TokenFormatDissector builds, as its parts: [("lit", text) | ("tok", token regex, captured)]"""
    assert rx.startswith("^") and rx.endswith("$"), rx
    parts = []
    i, n = 1, len(rx) - 1
    while i < n:
        if rx.startswith("\\Q", i):
            j = rx.index("\\E", i + 2)
            parts.append(("lit", rx[i + 2:j]))
            i = j + 2
            continue
        assert rx[i] == "(", (rx, i)
        depth, j = 0, i
        while True:
            if rx[j] == "\\":
                j += 2
                continue
            if rx[j] == "[":
                j = rx.index("]", j + 2)
            elif rx[j] == "(":
                depth += 1
            elif rx[j] == ")":
                depth -= 1
                if depth == 0:
                    break
            j += 1
        captured = not rx.startswith("(?:", i)
        parts.append(("tok", rx[i + (1 if captured else 3):j], captured))
        i = j + 1
    return parts


class Ref:
    """one format's reference: the regex the oracle prints for it when exactly GROUPS are requested, run by `re`"""

    def __init__(self, oracle, name):
        self.name = name
        self.logformat, self.groups = FORMATS[name]
        self.java = oracle.Oracle(self.logformat, self.groups).regex()
        self.python = java_to_py(self.java)
        self.re = re.compile(self.python, re.ASCII)
        assert self.re.groups == len(self.groups), (name, self.java)
        self.parts = split_regex(self.java)
        assert all(p[2] for p in self.parts if p[0] == "tok"), (name, self.java)  # every token requested

    def expect(self, line):
        """None: no match; else the tuple of group texts.  Lines outside ASCII or with a line terminator are
        refused: the batch splitter never yields the one, the device sends the other to FALLBACK by design."""
        s = line.decode("ascii")
        assert "\n" not in s and "\r" not in s, line
        m = self.re.search(s)
        return None if m is None else m.groups()

    def record(self, groups):
        """the record of a match: one value per group, "-" as null (decodeExtractedValue)"""
        return {p: [None if g == "-" else g] for p, g in zip(self.groups, groups)}


# ---------------------------------------------------------------- a handle's corpus and its expectation
class Case:
    """a handle (one format, or the formats of MULTI) with its corpus and, per line, the expectation of `re`:
    None (no format matches) or (index of the one format that matches, its group texts)"""

    def __init__(self, oracle, name):
        import regex_corpus
        self.name = name
        self.logformat, self.fields = logformat(name), fields(name)
        self.refs = [Ref(oracle, f) for f in MULTI.get(name, (name,))]
        if name in MULTI:
            # half a corpus of each format in one seeded order; without the VT / FF lines: an undecided line
            # leaves the routing state unknown, which is test_sticky_routing's subject and not this one's
            a, b = (regex_corpus.build(r.parts, n_lines=regex_corpus.N_LINES // 2) for r in self.refs)
            b = [l for l in b if l not in set(a)]
            self.lines = [l for _, l in regex_corpus.interleave(a, b) if b"\x0b" not in l and b"\x0c" not in l]
        else:
            self.lines = regex_corpus.build(self.refs[0].parts)
        self.short = regex_corpus.short_lines(self.refs[0].parts)
        self.want = [self.expect(l) for l in self.lines]

    def expect(self, line):
        hits = [(k, g) for k, g in ((k, r.expect(line)) for k, r in enumerate(self.refs)) if g is not None]
        assert len(hits) <= 1, ("a line that two formats of the handle match", self.name, line)
        return hits[0] if hits else None

    def record(self, want):
        return self.refs[want[0]].record(want[1])

    def same(self, want, record):
        """the record of a line against the expectation: one value per group of the format that matches, and
        nothing else (a several-format handle's record holds only the routed format's paths)"""
        return record == self.record(want)


_CASES = {}


def case(oracle, name):
    if name not in _CASES:
        _CASES[name] = Case(oracle, name)
    return _CASES[name]


NAMES = list(FORMATS) + list(MULTI)
