"""TEST-ONLY corpus of the GeoIP dissectors' tests: a small MaxMind DB writer
(from the format specification), synthetic databases that cover the record
sizes, both ip_versions, pointers of all four sizes, every data type and the
tree shapes where a walk can go wrong, and about 1,000 log lines whose
client address is every form the address parser decides or refuses."""
import ipaddress
import os
import random
import struct

MARKER = b"\xab\xcd\xefMaxMind.com"


# ---- typed values of the writer (a plain int is a uint32, a float a double)
class U16(int): pass
class U64(int): pass
class U128(int): pass
class I32(int): pass
class F32(float): pass
class Raw(bytes): pass      # the "bytes" type


class Ptr:
    """a pointer of the given size class (0..3) to data offset off"""
    def __init__(self, off, ss):
        self.off, self.ss = off, ss


def _ctrl(typ, size):
    if size < 29:
        s, extra = size, b""
    elif size < 285:
        s, extra = 29, bytes([size - 29])
    elif size < 65821:
        s, extra = 30, (size - 285).to_bytes(2, "big")
    else:
        s, extra = 31, (size - 65821).to_bytes(3, "big")
    if typ <= 7:
        return bytes([(typ << 5) | s]) + extra
    return bytes([s, typ - 7]) + extra


def _uint(v, width):
    raw = int(v).to_bytes(width, "big").lstrip(b"\0")
    return raw


def encode(v):
    if isinstance(v, Ptr):
        base = (0, 2048, 526336, 0)[v.ss]
        x = v.off - base
        assert x >= 0
        if v.ss == 3:
            return bytes([(1 << 5) | (3 << 3)]) + x.to_bytes(4, "big")
        n = v.ss + 1
        assert x < 1 << (8 * n + 3)
        return bytes([(1 << 5) | (v.ss << 3) | (x >> (8 * n))]) + (x & ((1 << (8 * n)) - 1)).to_bytes(n, "big")
    if isinstance(v, bool):
        return bytes([int(v), 14 - 7])
    if isinstance(v, Raw):
        return _ctrl(4, len(v)) + bytes(v)
    if isinstance(v, str):
        b = v.encode("utf-8")
        return _ctrl(2, len(b)) + b
    if isinstance(v, F32):
        return _ctrl(15, 4) + struct.pack(">f", v)
    if isinstance(v, float):
        return _ctrl(3, 8) + struct.pack(">d", v)
    if isinstance(v, U16):
        r = _uint(v, 2)
        return _ctrl(5, len(r)) + r
    if isinstance(v, U64):
        r = _uint(v, 8)
        return _ctrl(9, len(r)) + r
    if isinstance(v, U128):
        r = _uint(v, 16)
        return _ctrl(10, len(r)) + r
    if isinstance(v, I32):
        r = (int(v) & 0xFFFFFFFF).to_bytes(4, "big")
        return _ctrl(8, 4) + r
    if isinstance(v, int):
        r = _uint(v, 4)
        return _ctrl(6, len(r)) + r
    if isinstance(v, dict):
        out = _ctrl(7, len(v))
        for k, x in v.items():
            out += encode(k) + encode(x)
        return out
    if isinstance(v, (list, tuple)):
        out = _ctrl(11, len(v))
        for x in v:
            out += encode(x)
        return out
    raise TypeError(type(v))


class Writer:
    """networks -> a MaxMind DB file.  data(value) appends a value to the data
    section and returns its offset (for records and for pointers)."""

    def __init__(self, ip_version, record_size, database_type):
        self.ip_version, self.record_size, self.database_type = ip_version, record_size, database_type
        self.section = bytearray()
        self.nodes = [[None, None]]  # child: None, ("n", index), ("d", data offset)

    def data(self, value):
        off = len(self.section)
        self.section += encode(value)
        return off

    def pad_to(self, off):
        """a filler "bytes" value so that the next value starts at or after off"""
        if len(self.section) < off:
            self.data(Raw(b"\0" * (off - len(self.section))))

    def insert(self, network, data_off):
        net = ipaddress.ip_network(network)
        bits, plen, value = net.max_prefixlen, net.prefixlen, int(net.network_address)
        if self.ip_version == 6 and bits == 32:  # an IPv4 network lives below ::/96
            bits, plen = 128, plen + 96
        assert plen >= 1 and (self.ip_version == 6 or bits == 32)
        node = 0
        for k in range(plen):
            bit = (value >> (bits - 1 - k)) & 1
            if k == plen - 1:
                assert self.nodes[node][bit] is None, network
                self.nodes[node][bit] = ("d", data_off)
                return
            c = self.nodes[node][bit]
            if c is None:
                self.nodes.append([None, None])
                c = self.nodes[node][bit] = ("n", len(self.nodes) - 1)
            assert c[0] == "n", network
            node = c[1]

    def to_bytes(self):
        n = len(self.nodes)
        rs = self.record_size

        def rec(c):
            v = n if c is None else c[1] if c[0] == "n" else n + 16 + c[1]
            assert v < 1 << rs, "record does not fit %d bits" % rs
            return v
        tree = bytearray()
        for left, right in self.nodes:
            a, b = rec(left), rec(right)
            if rs == 24:
                tree += a.to_bytes(3, "big") + b.to_bytes(3, "big")
            elif rs == 28:
                tree += (a & 0xFFFFFF).to_bytes(3, "big") + bytes([((a >> 24) << 4) | (b >> 24)]) + (b & 0xFFFFFF).to_bytes(3, "big")
            else:
                tree += a.to_bytes(4, "big") + b.to_bytes(4, "big")
        meta = {"binary_format_major_version": U16(2), "binary_format_minor_version": U16(0),
                "build_epoch": U64(1600000000), "database_type": self.database_type,
                "description": {"en": "synthetic test database"}, "ip_version": U16(self.ip_version),
                "languages": ["en"], "node_count": n, "record_size": U16(rs)}
        return bytes(tree) + b"\0" * 16 + bytes(self.section) + MARKER + encode(meta)


# ---- records ----------------------------------------------------------------
def city(name, iso="NL", **kw):
    r = {"continent": {"code": "EU", "geoname_id": 6255148, "names": {"de": "Europa", "en": "Europe"}},
         "country": {"geoname_id": 2750405, "iso_code": iso, "names": {"en": "Country " + iso, "fr": "Pays"},
                     "confidence": U16(42), "is_in_european_union": True},
         "city": {"confidence": U16(1), "geoname_id": 1234, "names": {"en": name}},
         "location": {"accuracy_radius": U16(4), "latitude": 52.5, "longitude": 5.75, "time_zone": "Europe/Amsterdam",
                      "metro_code": U16(5), "average_income": 6, "population_density": 7},
         "postal": {"code": "1187", "confidence": U16(2)},
         "subdivisions": [{"iso_code": "XX", "names": {"en": "Outer"}}, {"iso_code": "NH", "names": {"en": "Noord " + name}}]}
    r.update(kw)
    return r


# every data type the format has, in keys no dissector reads (the reader skips them)
EXTRA = {"t_utf8": "text", "t_double": 1.25, "t_bytes": Raw(b"\x01\x02\xff"), "t_u16": U16(65535), "t_u32": 4000000000,
         "t_map": {"a": {"b": {"c": [1, 2, {"d": "e"}]}}}, "t_i32": I32(-7), "t_u64": U64((1 << 64) - 1),
         "t_u128": U128((1 << 127) + 5), "t_array": ["x", ["y", []], {}], "t_true": True, "t_false": False,
         "t_float": F32(1.5), "t_long_string": "s" * 300}

SPARSE = [
    {"country": {"iso_code": "ZZ"}},                                           # most fields absent: delivered null
    {"continent": {"names": {"de": "Europa"}}, "city": {"names": {}}},         # names without "en"
    {"location": {"latitude": F32(-12.25), "longitude": 1.0e-5}, "subdivisions": []},
    {"location": {"latitude": 1.2345678e7, "longitude": -0.0, "accuracy_radius": U16(0)},
     "country": {"is_in_european_union": False, "confidence": I32(-3), "names": {"en": "Zürich ☃"}}},
    {"city": {"geoname_id": U64(1 << 40), "confidence": "high"}, "postal": {"code": 1187}},  # other types than the getters'
    {},
]


def _records(w, n, with_extra=True):
    """n distinct City records in w's data section: their offsets"""
    offs = []
    for k in range(n):
        if k % 4 == 3:
            r = dict(SPARSE[(k // 4) % len(SPARSE)])
            r["tag"] = k  # (distinct bytes, distinct records)
        else:
            r = city("City%d" % k, iso="C%d" % (k % 7))
            if k % 3 == 0:
                del r["subdivisions"]
            if k % 5 == 0:
                del r["location"]["metro_code"]
        if with_extra and k % 2 == 0:
            r = dict(EXTRA, **r)
        offs.append(w.data(r))
    return offs


def db_v4_24():
    """ip_version 4, 24-bit records: data at prefix lengths 1, 8, 31 and 32"""
    w = Writer(4, 24, "Synthetic-City")
    offs = _records(w, 8)
    nets = ["128.0.0.0/1", "10.0.0.0/8", "1.2.3.4/31", "1.2.3.6/32", "0.0.0.0/32", "127.255.255.255/32", "80.100.0.0/16"]
    for k, n in enumerate(nets):
        w.insert(n, offs[k])
    return w.to_bytes(), nets


def db_v6_28():
    """ip_version 6, 28-bit records: IPv4 below ::/96, IPv6 data at prefix
    lengths 96, 97, 127 and 128, different data at ::ffff:1.2.3.4 and at
    ::1.2.3.4 (the mapped text is looked up as IPv4: the latter's)"""
    w = Writer(6, 28, "Synthetic-City")
    shared = w.data("Shared City Name")          # offset 0: pointers of sizes 0 and 3 reach it
    offs = _records(w, 12)
    w.pad_to(2048)
    far = w.data({"en": "Far Names"})            # >= 2048: a size-1 pointer
    ptr_rec = w.data({"city": {"names": {Ptr(far + 1, 1): Ptr(shared, 0)}, "geoname_id": 77},
                      "country": {"names": Ptr(far, 1), "iso_code": Ptr(shared, 3)},
                      Ptr(shared, 0): "a pointer as a key"})
    nets = ["1.2.3.4/32", "80.100.0.0/16", "255.255.255.255/32", "0.0.0.0/32", "10.0.0.0/8",
            "::ffff:1.2.3.4/128", "2001:db8::/96", "2001:db8:1::8000:0/97", "2001:db8:2::2/127", "2001:db8:3::1/128",
            "2001:980::/32", "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff/128", "1::/16"]
    for k, n in enumerate(nets[:-1]):
        w.insert(n, offs[k])
    w.insert(nets[-1], ptr_rec)
    return w.to_bytes(), nets


def db_v6_32_big():
    """ip_version 6, 32-bit records, no ::/96 at all (every IPv4 address is
    none), a data section past 526336 bytes: a size-2 pointer"""
    w = Writer(6, 32, "Synthetic-City")
    shared = w.data("Shared")
    offs = _records(w, 4)
    w.pad_to(526336)
    far = w.data("Beyond half a megabyte")
    rec = w.data({"city": {"names": {"en": Ptr(far, 2)}}, "country": {"iso_code": Ptr(shared, 3)},
                  "continent": {"code": Ptr(far, 3)}})
    nets = ["2001::/16", "2a00::/12", "fe80::/64", "8000::/2"]
    for k, n in enumerate(nets[:-1]):
        w.insert(n, offs[k])
    w.insert(nets[-1], rec)
    return w.to_bytes(), nets


def db_v6_leaf64():
    """ip_version 6 whose ::/64 is a data record: the IPv4 start is already a
    leaf, the walk must stop before its first step"""
    w = Writer(6, 24, "Synthetic-City")
    offs = _records(w, 3, with_extra=False)
    nets = ["::/64", "2001:db8::/32", "0:0:0:1::/64"]
    for k, n in enumerate(nets):
        w.insert(n, offs[k])
    return w.to_bytes(), nets


def db_asn():
    w = Writer(6, 24, "Synthetic-ASN")
    recs = [{"autonomous_system_number": 4444, "autonomous_system_organization": "Basjes Global Network"},
            {"autonomous_system_number": U64(4200000000), "isp": "unused here"},
            {"autonomous_system_organization": "No Number"}]
    offs = [w.data(r) for r in recs]
    nets = ["80.100.0.0/16", "2001:db8::/32", "10.0.0.0/8"]
    for k, n in enumerate(nets):
        w.insert(n, offs[k])
    return w.to_bytes(), nets


CITY_DBS = {"v4_24": db_v4_24, "v6_28": db_v6_28, "v6_32_big": db_v6_32_big, "v6_leaf64": db_v6_leaf64}


def write_db(tmpdir, name):
    """the synthetic database `name` as a file under tmpdir: (path, bytes, its networks)"""
    data, nets = (CITY_DBS.get(name) or {"asn": db_asn}[name])()
    path = os.path.join(str(tmpdir), name + ".mmdb")
    with open(path, "wb") as f:
        f.write(data)
    return path, data, nets


# ---- lines --------------------------------------------------------------------
LOGFORMAT = '%h %l %u %t "%r" %>s %b'
FIXED_HOSTS = [
    "0.0.0.0", "255.255.255.255", "1.2.3.4", "1.2.3.5", "1.2.3.6", "1.2.3.7", "127.0.0.1", "127.255.255.255",
    "128.0.0.0", "10.255.0.1", "80.100.47.45", "9.9.9.9",
    "::", "::1", "1::", "1:0:0:0:0:0:0:1", "2001:db8:0:0:0:0:0:1", "2001:0db8:0000:0000:0000:0000:0000:0001",
    "2001:DB8::ABCD", "2001:db8:1::8000:1", "2001:db8:1::7fff:ffff", "2001:db8:2::2", "2001:db8:2::3", "2001:db8:2::4",
    "2001:db8:3::1", "2001:db8:3::2", "2001:980:91c0:1:21c:c0ff:fe06:e580", "fe80::1", "2a01::1", "8000::",
    "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "FFFF:FFFF:FFFF:FFFF:FFFF:FFFF:FFFF:FFFF",
    "::1.2.3.4", "::ffff:1.2.3.4", "::FFFF:102:304", "::ffff:80.100.47.45", "0:0:0:0:0:ffff:1.2.3.4",
    "2001:db8::1.2.3.4", "1:2:3:4:5:6:1.2.3.4", "1:2:3:4:5:6:7::", "::2:3:4:5:6:7:8", "0:0:0:1::5", "64:ff9b::1.2.3.4",
    "-",
]
# values the address parser leaves to the reference (FALLBACK)
UNDECIDED_HOSTS = [
    "localhost", "www.example.com", "host-1.example", "1.2.3", "1.2.3.4.5", "01.2.3.4", "1.2.3.04", "1.2.3.256",
    "1.2.3.", ".1.2.3", "1..2.3", "1234", "256.1.1.1", "1.2.3.4a", "0x7f.1", "1::2::3", "1:2:3:4:5:6:7:8:9",
    "12345::1", "[::1]", "fe80::1%eth0", ":1:2:3:4:5:6:7", "1:2:3:4:5:6:7:", "1:2:3:4:5:6:7", ":::", "::g",
    "1:2:3:4:5:6:7:1.2.3.4", "::1.2.3", "::01.2.3.4", "1.2.3.4::", "::1.2.3.4:5", "1:2:3:4:5:6:7:8::",
    "2001:db8:aaaa:bbbb:cccc:dddd:eeee:255.255.255.255x", "a" * 46, "1111:2222:3333:4444:5555:6666:123.123.123.1234",
]


def _line(host, k=0, path="/index.html"):
    return '%s - - [10/Oct/2023:13:55:%02d +0200] "GET %s?k=%d HTTP/1.1" 200 %d' % (host, k % 60, path, k, 100 + k)


def hosts(seed=20261021, n=1000):
    """about n client values: the fixed forms, the planted undecided values,
    random addresses inside and outside the synthetic networks in several
    spellings"""
    rnd = random.Random(seed)
    out = list(FIXED_HOSTS) + list(UNDECIDED_HOSTS)
    v4_nets = ["10.0.0.0/8", "80.100.0.0/16", "1.2.3.4/30", "128.0.0.0/1", "0.0.0.0/8"]
    v6_nets = ["2001:db8::/96", "2001:db8:1::/64", "2001:db8:2::/124", "2001:980::/32", "1::/16", "2a00::/12",
               "fe80::/64", "::/64", "0:0:0:1::/64", "8000::/2", "::ffff:0:0/96"]
    while len(out) < n - 8:
        r = rnd.random()
        if r < 0.45:
            net = ipaddress.ip_network(rnd.choice(v4_nets))
            a = ipaddress.IPv4Address(int(net.network_address) + rnd.randrange(net.num_addresses))
            if rnd.random() < 0.2:
                a = ipaddress.IPv4Address(rnd.getrandbits(32))
            out.append(str(a))
        elif r < 0.9:
            net = ipaddress.ip_network(rnd.choice(v6_nets))
            a = ipaddress.IPv6Address(int(net.network_address) + rnd.randrange(net.num_addresses))
            if rnd.random() < 0.2:
                a = ipaddress.IPv6Address(rnd.getrandbits(128))
            form = rnd.random()
            s = str(a) if form < 0.5 else a.exploded if form < 0.7 else str(a).upper() if form < 0.85 else None
            if s is None:  # the last two groups as a dotted quad
                head = a.exploded.rsplit(":", 2)[0]
                s = head + ":" + str(ipaddress.IPv4Address(int(a) & 0xFFFFFFFF))
            out.append(s)
        elif r < 0.95:
            out.append("-")
        else:
            out.append(rnd.choice(UNDECIDED_HOSTS))
    return out


BAD_LINES = ["this is not a log line", '1.2.3.4 - - [bad time] "GET / HTTP/1.1" 200 1', ""]


def corpus(seed=20261021, n=1000):
    """[(line bytes, host value or None for a line that never reaches the
    dissector: BAD, or FALLBACK for another reason)]"""
    hs = hosts(seed, n)
    rnd = random.Random(seed + 1)
    rnd.shuffle(hs)
    out = [(_line(h, k).encode(), h) for k, h in enumerate(hs)]
    # BAD lines, and lines that are FALLBACK whatever is requested (longer than the device's line limit)
    for k, b in enumerate(BAD_LINES):
        out.insert(50 + 97 * k, (b.encode(), None))
    for k in range(3):
        out.insert(200 + 211 * k, (_line("80.100.47.45", k, "/" + "x" * 9000).encode(), None))
    return out


def data_of(lines):
    return b"".join(l + b"\n" for l, _ in lines)
