"""TEST-ONLY independent restatement of the GeoIP dissectors
(hp/dissectors/geoip/*.java on geoip2 2.12.0 / maxmind-db): its own MaxMind DB
reader written from the format specification, its own address rules built on
the ipaddress module, and its own field extraction.  Shares no code with the
C++ (logparser_amd/csrc/lp_mmdb.h, lp_geoip.h, plan.cpp)."""
import ipaddress
import re
import struct

MARKER = b"\xab\xcd\xefMaxMind.com"


class Reader:
    def __init__(self, data):
        self.buf = bytes(data)
        at = self.buf.rfind(MARKER)
        if at < 0:
            raise ValueError("no metadata marker")
        self.base = at + len(MARKER)
        self.meta, _ = self._decode(0)
        self.node_count = self.meta["node_count"]
        self.record_size = self.meta["record_size"]
        self.ip_version = self.meta["ip_version"]
        self.database_type = self.meta["database_type"]
        self.tree_bytes = self.node_count * self.record_size * 2 // 8
        self.base = self.tree_bytes + 16

    # -- data section -------------------------------------------------------
    def _decode(self, pos):
        """(value, position after it) of the field at data offset pos"""
        b = self.buf
        ctrl = b[self.base + pos]
        pos += 1
        typ = ctrl >> 5
        if typ == 1:  # pointer
            ss = (ctrl >> 3) & 3
            raw = b[self.base + pos:self.base + pos + ss + 1]
            pos += ss + 1
            if ss == 0:
                ptr = ((ctrl & 7) << 8) | raw[0]
            elif ss == 1:
                ptr = 2048 + (((ctrl & 7) << 16) | int.from_bytes(raw, "big"))
            elif ss == 2:
                ptr = 526336 + (((ctrl & 7) << 24) | int.from_bytes(raw, "big"))
            else:
                ptr = int.from_bytes(raw, "big")
            return self._decode(ptr)[0], pos
        if typ == 0:
            typ = 7 + b[self.base + pos]
            pos += 1
        size = ctrl & 31
        if typ != 14 and size >= 29:
            n = size - 28
            extra = int.from_bytes(b[self.base + pos:self.base + pos + n], "big")
            pos += n
            size = extra + (29, 285, 65821)[n - 1]
        raw = b[self.base + pos:self.base + pos + size]
        if typ == 2:
            return raw.decode("utf-8"), pos + size
        if typ == 3:
            return struct.unpack(">d", raw)[0], pos + size
        if typ == 4:
            return raw, pos + size
        if typ in (5, 6, 9, 10):
            return int.from_bytes(raw, "big"), pos + size
        if typ == 7:
            out = {}
            for _ in range(size):
                k, pos = self._decode(pos)
                v, pos = self._decode(pos)
                out.setdefault(k, v)
            return out, pos
        if typ == 8:
            v = int.from_bytes(raw, "big")
            return (v - (1 << 32) if size == 4 and v >> 31 else v), pos + size
        if typ == 11:
            out = []
            for _ in range(size):
                v, pos = self._decode(pos)
                out.append(v)
            return out, pos
        if typ == 14:
            return size != 0, pos
        if typ == 15:
            return struct.unpack(">f", raw)[0], pos + size
        raise ValueError("type %d" % typ)

    # -- search tree --------------------------------------------------------
    def _record(self, node, side):
        rs = self.record_size
        p = node * rs // 4
        b = self.buf
        if rs == 24:
            return int.from_bytes(b[p + 3 * side:p + 3 * side + 3], "big")
        if rs == 28:
            mid = b[p + 3]
            if side == 0:
                return ((mid >> 4) << 24) | int.from_bytes(b[p:p + 3], "big")
            return ((mid & 15) << 24) | int.from_bytes(b[p + 4:p + 7], "big")
        return int.from_bytes(b[p + 4 * side:p + 4 * side + 4], "big")

    def lookup(self, addr):
        """the record (a dict) of an ipaddress address, or None"""
        bits = addr.max_prefixlen
        value = int(addr)
        node = 0
        if bits == 32 and self.ip_version == 6:
            for _ in range(96):
                if node >= self.node_count:
                    break
                node = self._record(node, 0)
        elif bits == 128 and self.ip_version == 4:
            raise ValueError("IPv6 address in an IPv4 database")
        for k in range(bits):
            if node >= self.node_count:
                break
            node = self._record(node, (value >> (bits - 1 - k)) & 1)
        if node <= self.node_count:  # "not found" (== node_count), or a tree deeper than the address
            return None
        return self._decode(node - self.node_count - 16)[0]


_QUAD = re.compile(r"^(0|[1-9][0-9]{0,2})\.(0|[1-9][0-9]{0,2})\.(0|[1-9][0-9]{0,2})\.(0|[1-9][0-9]{0,2})$")


def parse_address(text):
    """InetAddress.getByName for the decided subset: an IPv4Address, an
    IPv6Address, or None (undecided: a host name or a legacy form)."""
    if not text or len(text) > 45 or any(c in text for c in "%[]/ "):
        return None
    m = _QUAD.match(text)
    if m:
        if all(int(g) <= 255 for g in m.groups()):
            return ipaddress.IPv4Address(text)
        return None
    if ":" not in text:
        return None
    # the groups must be 1-4 hex digits; a dotted quad only as the last two groups, in the strict form
    tail = text.rsplit(":", 1)[1]
    if "." in tail:
        mq = _QUAD.match(tail)
        if not mq or not all(int(g) <= 255 for g in mq.groups()):
            return None
    if not re.match(r"^[0-9A-Fa-f:.]+$", text):
        return None
    try:
        a = ipaddress.IPv6Address(text)
    except ValueError:
        return None
    if a.ipv4_mapped is not None:  # the JDK hands back an Inet4Address for ::ffff:a.b.c.d
        return a.ipv4_mapped
    return a


# (output "TYPE:name", kind, how to read it from the record)
def _names_en(d):
    return None if d is None else (d.get("names") or {}).get("en")


def _sub(rec):
    subs = rec.get("subdivisions") or []
    return subs[-1] if subs else {}


COUNTRY = [
    ("STRING:continent.name", "S", lambda r: _names_en(r.get("continent", {}))),
    ("STRING:continent.code", "S", lambda r: r.get("continent", {}).get("code")),
    ("STRING:country.name", "S", lambda r: _names_en(r.get("country", {}))),
    ("STRING:country.iso", "S", lambda r: r.get("country", {}).get("iso_code")),
    ("NUMBER:country.getconfidence", "L", lambda r: r.get("country", {}).get("confidence")),
    ("BOOLEAN:country.isineuropeanunion", "L", lambda r: 1 if r.get("country", {}).get("is_in_european_union") is True else 0),
]
CITY = COUNTRY + [
    ("STRING:subdivision.name", "S", lambda r: _names_en(_sub(r))),
    ("STRING:subdivision.iso", "S", lambda r: _sub(r).get("iso_code")),
    ("STRING:city.name", "S", lambda r: _names_en(r.get("city", {}))),
    ("NUMBER:city.confidence", "L", lambda r: r.get("city", {}).get("confidence")),
    ("NUMBER:city.geonameid", "L", lambda r: r.get("city", {}).get("geoname_id")),
    ("STRING:postal.code", "S", lambda r: r.get("postal", {}).get("code")),
    ("NUMBER:postal.confidence", "L", lambda r: r.get("postal", {}).get("confidence")),
    ("STRING:location.latitude", "D", lambda r: r.get("location", {}).get("latitude")),
    ("STRING:location.longitude", "D", lambda r: r.get("location", {}).get("longitude")),
    ("STRING:location.timezone", "S", lambda r: r.get("location", {}).get("time_zone")),
    ("NUMBER:location.accuracyradius", "L", lambda r: r.get("location", {}).get("accuracy_radius")),
    ("NUMBER:location.averageincome", "L?", lambda r: r.get("location", {}).get("average_income")),
    ("NUMBER:location.metrocode", "L?", lambda r: r.get("location", {}).get("metro_code")),
    ("NUMBER:location.populationdensity", "L?", lambda r: r.get("location", {}).get("population_density")),
]
ASN = [
    ("ASN:asn.number", "L", lambda r: r.get("autonomous_system_number")),
    ("STRING:asn.organization", "S", lambda r: r.get("autonomous_system_organization")),
]
ISP = ASN + [
    ("STRING:isp.name", "S", lambda r: r.get("isp")),
    ("STRING:isp.organization", "S", lambda r: r.get("organization")),
]
CLASSES = {"GeoIPCountryDissector": COUNTRY, "GeoIPCityDissector": CITY, "GeoIPASNDissector": ASN,
           "GeoIPISPDissector": ISP}
CASTS = {"S": 1, "L": 3, "L?": 3, "D": 5}  # STRING 1 | LONG 2 | DOUBLE 4


def java_double(x):
    """Double.toString of a finite double (the shortest round-trip digits)"""
    if x == 0:
        return "-0.0" if str(x).startswith("-") else "0.0"
    r = repr(float(x))
    mant, _, exp = r.partition("e")
    neg = mant.startswith("-")
    mant = mant.lstrip("-")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0") or "0"
    # decimal exponent of the first significant digit
    e10 = (int(exp) if exp else 0) + len(ip) - 1
    if ip.strip("0") == "":
        e10 = (int(exp) if exp else 0) - (len(fp) - len(fp.lstrip("0"))) - 1
    digits = digits.rstrip("0") or "0"
    if -3 <= e10 < 7:
        if e10 >= 0:
            d = digits.ljust(e10 + 1, "0")
            out = d[:e10 + 1] + "." + (d[e10 + 1:] or "0")
        else:
            out = "0." + "0" * (-e10 - 1) + digits
    else:
        out = digits[0] + "." + (digits[1:] or "0") + "E" + str(e10)
    return ("-" if neg else "") + out


def dissect(reader, cls, text):
    """What the class delivers for the value text: None when the line is the
    reference's (FALLBACK), else {output: value} -- a str, an int, None for a
    delivered null; a DOUBLE output is its Double.toString text.  "-" is the
    caller's null: pass None."""
    if text is None or text == "":
        return {}
    a = parse_address(text)
    if a is None:
        return None
    if a.version == 6 and reader.ip_version == 4:
        return None
    rec = reader.lookup(a)
    if rec is None:
        return {}
    out = {}
    for name, kind, get in CLASSES[cls]:
        v = get(rec)
        if kind == "S" and not isinstance(v, str):
            v = None
        if kind in ("L", "L?") and (isinstance(v, bool) or not isinstance(v, int)):
            v = None
        if kind == "D":
            v = java_double(v) if isinstance(v, float) else None
        if v is None and kind == "L?":
            continue
        out[name] = v
    return out
