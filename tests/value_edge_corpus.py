"""Value-edge corpora: inputs at the edges of the conversion code (calendar,
Long.parseLong, ConvertSecondsWithMillisString, Double.parseDouble, Long.toString,
BinaryIPDissector) with expectations computed here from the generating
parameters with datetime / calendar / int / float -- never from the engine,
the oracle or the host table.  Shared by test_value_edges.py (oracle, emu,
setters, the stand-alone program of csrc/lp_value.h) and
test_value_edges_gpu.py (the device table).

Time corpus: 26 years x 17 days x 8 offsets x 4 times = 14 144 instants,
rendered in the Apache %t, $time_iso8601 and strftime "%F %T %z" layouts,
plus the strftime %s inputs.  A line whose local or UTC day is outside
datetime.date's range has no expectation; year_10000() derives the same set
from the parameters alone.

Number corpus: an NGINX format of $body_bytes_sent, $request_time,
$upstream_response_time, $binary_remote_addr and $realip_remote_port.  The
last one is there for the sign: among the tokens with a LONG cast the
regexes of the first four admit digits only ([0-9]+, the "\\xHH" quadruple),
so Long.parseLong's sign branch is unreachable from them; $realip_remote_port
(PORT, casts STRING | LONG, regex .*?) delivers any text, signs included.
"""
import calendar
import datetime
import random
import re

# ------------------------------------------------------------------ time
YEARS = [1000, 1001, 1582, 1899, 1900, 1901, 1968, 1969, 1970, 1971, 1972, 1999, 2000, 2001, 2004, 2015, 2016, 2020,
         2021, 2026, 2099, 2100, 2101, 2400, 9998, 9999]
# (month, day as written: 29-31 Feb and 31 Apr are clamped by ResolverStyle.SMART)
DAYS = [(12, 27), (12, 28), (12, 29), (12, 30), (12, 31), (1, 1), (1, 2), (1, 3), (1, 4), (1, 5),
        (2, 28), (2, 29), (2, 30), (2, 31), (3, 1), (4, 31), (6, 30)]
OFFSETS = ["-1800", "-1200", "-0001", "+0000", "+0001", "+0530", "+1400", "+1800"]
TIMES = [(0, 0, 0), (23, 59, 59), (24, 0, 0), (12, 30, 15)]
EPOCH_INPUTS = [0, 86399, 86400, 951782400, 4107542400, 253402300799, 253402300800]

MONTHS = ["January", "February", "March", "April", "May", "June", "July", "August", "September", "October",
          "November", "December"]
EPOCH_ORDINAL = datetime.date(1970, 1, 1).toordinal()
MAX_ORDINAL = datetime.date.max.toordinal()  # 9999-12-31

_T = "request.receive.time."
# (path, column type, key of the expectation) for the local group; TIME_FIELDS adds _utc and the epoch
_GROUP = [("TIME.YEAR:" + _T + "year", int, "year"), ("TIME.MONTH:" + _T + "month", int, "month"),
          ("TIME.DAY:" + _T + "day", int, "day"), ("TIME.HOUR:" + _T + "hour", int, "hour"),
          ("TIME.MINUTE:" + _T + "minute", int, "minute"), ("TIME.SECOND:" + _T + "second", int, "second"),
          ("TIME.WEEK:" + _T + "weekofweekyear", int, "weekofweekyear"), ("TIME.YEAR:" + _T + "weekyear", int, "weekyear"),
          ("TIME.DATE:" + _T + "date", str, "date"), ("TIME.TIME:" + _T + "time", str, "time"),
          ("TIME.MONTHNAME:" + _T + "monthname", str, "monthname")]
TIME_FIELDS = _GROUP + [(p + "_utc", t, k + "_utc") for p, t, k in _GROUP] + [("TIME.EPOCH:" + _T + "epoch", int, "epoch")]

APACHE_FMT = "combined"
ISO_FMT = '$remote_addr - - [$time_iso8601] "$request" $status'
STRF_FMT = '%h [%{%F %T %z}t] "%r"'
EPOCH_FMT = '%h [%{%s}t] "%r"'
LAYOUTS = ("apache", "iso", "strf", "epoch")
FORMATS = {"apache": APACHE_FMT, "iso": ISO_FMT, "strf": STRF_FMT, "epoch": EPOCH_FMT}


def instants():
    """[(year, month, day, hour, minute, second, offset text)] in a fixed order"""
    return [(y, mo, d, h, mi, s, off) for y in YEARS for mo, d in DAYS for off in OFFSETS for h, mi, s in TIMES]


def offset_seconds(off):
    return (-1 if off[0] == "-" else 1) * (int(off[1:3]) * 3600 + int(off[3:5]) * 60)


def _fields_of(total, suffix, out):
    """the calendar fields of `total` seconds since ordinal 0, 00:00; False outside datetime.date"""
    o, sod = divmod(total, 86400)
    if not 1 <= o <= MAX_ORDINAL:
        return False
    d = datetime.date.fromordinal(o)
    iso = d.isocalendar()
    h, mi, s = sod // 3600, sod // 60 % 60, sod % 60
    out.update({"year" + suffix: d.year, "month" + suffix: d.month, "day" + suffix: d.day, "hour" + suffix: h,
                "minute" + suffix: mi, "second" + suffix: s, "weekofweekyear" + suffix: iso[1], "weekyear" + suffix: iso[0],
                "date" + suffix: "%04d-%02d-%02d" % (d.year, d.month, d.day), "time" + suffix: "%02d:%02d:%02d" % (h, mi, s),
                "monthname" + suffix: MONTHS[d.month - 1]})
    return True


def expect_local(local_total, off_s):
    """{key: value} of a local time (seconds since ordinal 0) at an offset; None outside datetime.date"""
    out = {}
    if not (_fields_of(local_total, "", out) and _fields_of(local_total - off_s, "_utc", out)):
        return None
    out["epoch"] = (local_total - off_s - EPOCH_ORDINAL * 86400) * 1000
    return out


def expect_instant(inst):
    """ordinal arithmetic: 24:00:00 and the offset never overflow a datetime"""
    y, mo, d, h, mi, s, off = inst
    day = min(d, calendar.monthrange(y, mo)[1])  # SMART: clamped to the month's length
    return expect_local(datetime.date(y, mo, day).toordinal() * 86400 + h * 3600 + mi * 60 + s, offset_seconds(off))


def year_10000(inst):
    """the local or UTC calendar year is 10000, from the parameters alone: 31 Dec 9999 at 24:00:00, or
    at a time a negative offset moves to or past the next UTC midnight"""
    y, mo, d, h, mi, s, off = inst
    return y == 9999 and (mo, d) == (12, 31) and (h == 24 or h * 3600 + mi * 60 + s - offset_seconds(off) >= 86400)


def render(layout, inst, k):
    """line k's bytes of an instant in a layout (k varies the client address)"""
    y, mo, d, h, mi, s, off = inst
    ip = "10.%d.%d.%d" % (k >> 16 & 255, k >> 8 & 255, k & 255)
    if layout == "apache":
        return ('%s - - [%02d/%s/%04d:%02d:%02d:%02d %s] "GET /t?k=%d HTTP/1.1" 200 %d "-" "edge/1.0"' %
                (ip, d, MONTHS[mo - 1][:3], y, h, mi, s, off, k, k)).encode()
    if layout == "iso":
        return ('%s - - [%04d-%02d-%02dT%02d:%02d:%02d%s:%s] "GET /t?k=%d HTTP/1.1" 200' %
                (ip, y, mo, d, h, mi, s, off[:3], off[3:], k)).encode()
    if layout == "strf":
        return ('%s [%04d-%02d-%02d %02d:%02d:%02d %s] "GET /t HTTP/1.1"' % (ip, y, mo, d, h, mi, s, off)).encode()
    raise ValueError(layout)


_TIME_CACHE = {}


def time_corpus(layout):
    """(LogFormat, lines, expectations, no_expectation, year_10000): expectations[i] a {key: value} or
    None; no_expectation the sorted indices of the None ones (outside datetime.date's range);
    year_10000 the sorted indices of the lines whose local or UTC year is 10000 (by the parameters
    alone).  The test asserts the two sets are the same.  Built once, shared, never modified."""
    if layout in _TIME_CACHE:
        return _TIME_CACHE[layout]
    if layout == "epoch":
        lines = [('10.0.0.%d [%d] "GET /t HTTP/1.1"' % (k, e)).encode() for k, e in enumerate(EPOCH_INPUTS)]
        exp = [expect_local(EPOCH_ORDINAL * 86400 + e, 0) for e in EPOCH_INPUTS]  # %s: no zone, UTC
        y10k = [k for k, e in enumerate(EPOCH_INPUTS) if e > 253402300799]  # 9999-12-31T23:59:59Z
    else:
        ins = instants()
        lines = [render(layout, inst, k) for k, inst in enumerate(ins)]
        exp = [expect_instant(inst) for inst in ins]
        y10k = [k for k, inst in enumerate(ins) if year_10000(inst)]
    _TIME_CACHE[layout] = (FORMATS[layout], lines, exp, [k for k, e in enumerate(exp) if e is None], y10k)
    return _TIME_CACHE[layout]


def interleave_short_lines(lines, seed):
    """the lines with runs of 70-260 one-byte lines between them (more than 64 line starts in a chunk:
    part of the corpus goes through the overflow kernel): (all lines, index of lines[k] among them)"""
    rng = random.Random(seed)
    out, at = [], []
    for k, l in enumerate(lines):
        if k % 150 == 5:
            out += [b"x"] * rng.randrange(70, 261)
        at.append(len(out))
        out.append(l)
    return out, at


# --------------------------------------------------------------- numbers
NUM_FMT = '$body_bytes_sent $request_time "$upstream_response_time" $binary_remote_addr [$realip_remote_port]'
LIST_ITEMS = 4  # list items 0..3 are requested; item 3 is never there

BYTES = ["0", "00", "0" * 35 + "12", "9223372036854775806", "9223372036854775807", "9223372036854775808",
         "9999999999999999999", "9" * 20, "18446744073709551616", "7", "1234567890"]
PORTS = ["+5", "-5", "-0", "+", "-", "-9223372036854775808", "-9223372036854775809", "80", "", "+9223372036854775807",
         "+9223372036854775808", "9223372036854775807", "65535", "+-5", "5-", " 5"]
BIN_BYTES = [-128, -100, -99, -10, -9, -1, 0, 9, 10, 99, 100, 127]
BAD_EVERY = 41  # a BAD line (a $request_time without its '.') at every row k with k % BAD_EVERY == 17


def _edge_decimals():
    v = ["999999999999999999.999", "9223372036854775.808", "18446744073709551.616", "0.999999999999999999",
         "000000000000000001.5", "9007199254740993.0", "0.000000000000000001", "0.1", "0.30000000000000004",
         "4503599627370496.5", "4503599627370497.5", "0.0", "0.000", "9.9", "9223372036854775.807",
         "9223372036854775.809", "18446744073709551.615", "1.000000000000000000", "123456789012345678.123456789012345678"]
    for e in range(53, 60):
        ulp = 1 << (e - 52)  # the spacing of doubles in [2^e, 2^(e+1)); an odd multiple of ulp/2 is a tie
        for i in ((1 << e) - 1, 1 << e, (1 << e) + 1, (1 << e) + ulp // 2, (1 << e) + 3 * ulp // 2):
            for f in ("0", "5", "500000000000000001", "499999999999999999"):
                v.append("%d.%s" % (i, f))
    return v


def _decimals(seed, n_random):
    """the edge values spread among seeded random I.F (1-18 digits each side): every 4th value an edge"""
    rng = random.Random(seed)
    edge = _edge_decimals()
    rnd = ["%s.%s" % ("".join(rng.choice("0123456789") for _ in range(rng.randint(1, 18))),
                      "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 18)))) for _ in range(n_random)]
    out = []
    while edge or rnd:
        if edge:
            out.append(edge.pop(0))
        out += rnd[:3]
        del rnd[:3]
    return out


def wrap64(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def secms(text):
    """ConvertSecondsWithMillisString: seconds * 1000 + the fraction read as an integer, Java long arithmetic"""
    i, f = text.split(".")
    return wrap64(int(i) * 1000 + int(f))


def java_long(text):
    """Long.parseLong of a text, None where it throws"""
    if text is None or not re.fullmatch(r"[+-]?[0-9]+", text, re.ASCII):
        return None
    v = int(text)
    return v if -(1 << 63) <= v < (1 << 63) else None


_UP = "nginxmodule.upstream.response.time"
_RT = "response.server.processing.time"


def num_paths():
    """the requested paths of NUM_FMT: every non-wildcard path, list items 0..LIST_ITEMS-1"""
    p = ["BYTES:response.body.bytes", "BYTESCLF:response.body.bytes", "IP:connection.client.host",
         "IP_BINARY:connection.client.host", "PORT:nginxmodule.realip.remote_port", "UPSTREAM_SECOND_MILLIS_LIST:" + _UP,
         "SECOND_MILLIS:" + _RT, "MILLISECONDS:" + _RT, "MICROSECONDS:" + _RT]
    for k in range(LIST_ITEMS):
        for part in ("value", "redirected"):
            p += ["%s:%s.%d.%s" % (t, _UP, k, part) for t in ("SECOND_MILLIS", "MILLISECONDS", "MICROSECONDS")]
    return p


def is_list_item(path):
    return path.startswith("SECOND_MILLIS:" + _UP + ".")


_NUM_CACHE = {}


def number_corpus(seed=20261020, n_random=2000):
    """(lines, expectations): expectations[k] None for a BAD line, else {path: None | str | int} -- a
    str is the delivered text, an int a delivered long.  Consecutive rows mix 1-character and
    20-character longs ("0.0" -> 0, "9223372036854775.808" -> -9223372036854775808), negative
    (wrapped) values, nulls (absent list items, the "-" port) and BAD lines.  Built once, shared,
    never modified."""
    key = (seed, n_random)
    if key in _NUM_CACHE:
        return _NUM_CACHE[key]
    dec = _decimals(seed, n_random)
    n = len(dec)
    lines, exp = [], []
    for k in range(n):
        by, port, rt = BYTES[k % len(BYTES)], PORTS[k % len(PORTS)], dec[(5 * k + 1) % n]
        if k % 16 in (3, 11):  # a 1-character and a 20-character long in every 16 rows
            rt = "0.0" if k % 16 == 3 else "9223372036854775.808"
        # 1, 2 or 3 upstreams; the second may have been redirected (" : "), the first never (the token's
        # regex).  Item 0 is dec[k]: every decimal is some row's first list item.
        servers = [(dec[k], None)]
        if k % 3 >= 1:
            servers.append((dec[(7 * k + 2) % n], dec[(11 * k + 3) % n] if k % 2 else None))
        if k % 3 == 2:
            servers.append((dec[(13 * k + 4) % n], None))
        up = ", ".join(v if r is None else v + " : " + r for v, r in servers)
        bb = [BIN_BYTES[(k // 4 + 5 * j) % len(BIN_BYTES)] for j in range(4)]
        bb[k % 4] = BIN_BYTES[k // 4 % len(BIN_BYTES)]  # each value in each position
        ip = "".join("\\x%02X" % (b & 255) for b in bb)
        if k % BAD_EVERY == 17:
            rt = rt.replace(".", "")
        lines.append(('%s %s "%s" %s [%s]' % (by, rt, up, ip, port)).encode())
        if k % BAD_EVERY == 17:
            exp.append(None)
            continue
        e = {"BYTES:response.body.bytes": by, "BYTESCLF:response.body.bytes": None if by == "0" else by,
             "IP:connection.client.host": "%d.%d.%d.%d" % tuple(bb), "IP_BINARY:connection.client.host": ip,
             "PORT:nginxmodule.realip.remote_port": None if port == "-" else port,
             "UPSTREAM_SECOND_MILLIS_LIST:" + _UP: up,
             "SECOND_MILLIS:" + _RT: rt, "MILLISECONDS:" + _RT: secms(rt), "MICROSECONDS:" + _RT: wrap64(secms(rt) * 1000)}
        for j in range(LIST_ITEMS):
            for part in ("value", "redirected"):
                t = None
                if j < len(servers):
                    t = servers[j][0] if part == "value" or servers[j][1] is None else servers[j][1]
                tail = "%s.%d.%s" % (_UP, j, part)
                e["SECOND_MILLIS:" + tail] = t
                e["MILLISECONDS:" + tail] = None if t is None else secms(t)
                e["MICROSECONDS:" + tail] = None if t is None else wrap64(secms(t) * 1000)
        exp.append(e)
    _NUM_CACHE[key] = (lines, exp)
    return _NUM_CACHE[key]


def column_expectation(path, typ, e):
    """(valid, value) of a table column of type typ (str / int / float) for an expectation e[path]:
    STRING the text (Long.toString of a long), LONG the long (Long.parseLong of a text, null where it
    throws), DOUBLE the long as a double or Double.parseDouble of a SECOND_MILLIS list item"""
    v = None if e is None else e[path]
    if v is None:
        return False, None
    if typ is str:
        return True, (str(v) if isinstance(v, int) else v).encode()
    if typ is int:
        v = v if isinstance(v, int) else java_long(v)
        return v is not None, v
    if isinstance(v, int):
        return True, float(v)
    if is_list_item(path):
        return True, float(v)
    raise ValueError("no DOUBLE expectation for " + path)


def decimal_strings():
    """every I.F text of the number corpus, in order of first appearance (the stand-alone program's input)"""
    return list(dict.fromkeys(_decimals(20261020, 2000)))
