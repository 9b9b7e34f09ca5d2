// A reader of the MaxMind DB file format 2.0 (the published specification:
// a binary search tree of 24 / 28 / 32-bit records, a data section, and a
// metadata map after the last "\xab\xcd\xefMaxMind.com"), for the GeoIP
// dissectors' compile-time preparation (plan.cpp).  Host code only.  Every
// read is bounds-checked against the section it belongs to; no exceptions;
// containers nest at most MMDB_MAX_DEPTH deep and a pointer may lead to a
// pointer at most MMDB_MAX_PTR times (a cycle of pointers ends there): a file
// that breaks a bound is invalid, never a crash.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "lp_geoip.h"

namespace lp {
namespace mmdb {

constexpr int MMDB_MAX_DEPTH = 16;
constexpr int MMDB_MAX_PTR = 4;

enum Type : int {
    T_POINTER = 1, T_UTF8 = 2, T_DOUBLE = 3, T_BYTES = 4, T_UINT16 = 5, T_UINT32 = 6, T_MAP = 7, T_INT32 = 8,
    T_UINT64 = 9, T_UINT128 = 10, T_ARRAY = 11, T_CACHE = 12, T_END = 13, T_BOOLEAN = 14, T_FLOAT = 15
};

// One decoded value.  Scalars hold their value; utf8 / bytes point into the
// section; a map / array holds its entry count (n) and where its first entry
// starts (pos).
struct Val {
    int type = 0;
    uint64_t u = 0;      // unsigned integers (uint128: the low 64 bits, hi the rest), boolean
    uint64_t hi = 0;
    int64_t i = 0;       // int32
    double d = 0;        // double, float
    const uint8_t* s = nullptr;
    uint32_t n = 0;      // bytes of a string, entries of a map / array
    size_t pos = 0;
};

// A data section: [p, p + len).  Pointers are offsets into it.
struct Section {
    const uint8_t* p = nullptr;
    size_t len = 0;
};

// The value whose control byte is at pos; pos moves past it (past the
// pointer itself when it is one, past the header of a map / array: its
// entries follow).  false: out of bounds or malformed.
inline bool decode(const Section& S, size_t& pos, Val& v, int ptr_depth = 0) {
    if (pos >= S.len) return false;
    const uint8_t ctrl = S.p[pos++];
    int type = ctrl >> 5;
    if (type == T_POINTER) {
        const uint32_t ss = (ctrl >> 3) & 3u, vvv = ctrl & 7u;
        if (pos + ss + 1 > S.len) return false;
        uint64_t t = 0;
        for (uint32_t k = 0; k <= ss; ++k) t = (t << 8) | S.p[pos + k];
        pos += ss + 1;
        if (ss == 0) t |= (uint64_t)vvv << 8;
        else if (ss == 1) t = (t | ((uint64_t)vvv << 16)) + 2048;
        else if (ss == 2) t = (t | ((uint64_t)vvv << 24)) + 526336;
        if (ptr_depth >= MMDB_MAX_PTR || t >= S.len) return false;
        size_t at = (size_t)t;
        return decode(S, at, v, ptr_depth + 1);  // (bounded: ptr_depth)
    }
    if (type == 0) {  // extended: the next byte + 7
        if (pos >= S.len) return false;
        type = 7 + S.p[pos++];
        if (type <= 7 || type > T_FLOAT) return false;
    }
    size_t size = ctrl & 31u;
    if (type != T_BOOLEAN && size >= 29) {
        const size_t extra = size - 28;  // 1, 2 or 3 bytes
        if (pos + extra > S.len) return false;
        size_t t = 0;
        for (size_t k = 0; k < extra; ++k) t = (t << 8) | S.p[pos + k];
        pos += extra;
        size = t + (extra == 1 ? 29 : extra == 2 ? 285 : 65821);
    }
    v = Val{};
    v.type = type;
    auto be = [&](size_t n, uint64_t& lo, uint64_t& hi) {
        lo = hi = 0;
        for (size_t k = 0; k < n; ++k) {
            hi = (hi << 8) | (lo >> 56);
            lo = (lo << 8) | S.p[pos + k];
        }
    };
    switch (type) {
    case T_UTF8: case T_BYTES:
        if (size > S.len - pos) return false;
        v.s = S.p + pos;
        v.n = (uint32_t)size;
        pos += size;
        return true;
    case T_DOUBLE: {
        if (size != 8 || pos + 8 > S.len) return false;
        uint64_t lo, hi;
        be(8, lo, hi);
        memcpy(&v.d, &lo, 8);
        pos += 8;
        return true;
    }
    case T_FLOAT: {
        if (size != 4 || pos + 4 > S.len) return false;
        uint64_t lo, hi;
        be(4, lo, hi);
        const uint32_t w = (uint32_t)lo;
        float f;
        memcpy(&f, &w, 4);
        v.d = (double)f;
        pos += 4;
        return true;
    }
    case T_UINT16: case T_UINT32: case T_UINT64: case T_UINT128: case T_INT32: {
        const size_t max = type == T_UINT16 ? 2 : type == T_UINT64 ? 8 : type == T_UINT128 ? 16 : 4;
        if (size > max || size > S.len - pos) return false;
        be(size, v.u, v.hi);
        if (type == T_INT32) v.i = (int64_t)(int32_t)(uint32_t)v.u;
        pos += size;
        return true;
    }
    case T_MAP: case T_ARRAY:
        if (size > S.len) return false;  // (every entry takes at least one byte)
        v.n = (uint32_t)size;
        v.pos = pos;
        return true;
    case T_BOOLEAN:
        v.u = size != 0;
        return true;
    default:  // the data cache container and the end marker never stand in a record
        return false;
    }
}

// The value of key in map m (m.type == T_MAP).  found = false when the map has
// no such key; the return value is false only for a malformed map.
inline bool map_get(const Section& S, const Val& m, const char* key, Val& out, bool& found, int depth = 0);

// pos past one value, entries of a container included (pointers are not followed)
inline bool skip_value(const Section& S, size_t& pos, int depth) {
    if (depth > MMDB_MAX_DEPTH || pos >= S.len) return false;
    if ((S.p[pos] >> 5) == T_POINTER) {
        pos += 2 + ((S.p[pos] >> 3) & 3u);
        return pos <= S.len;
    }
    Val v;
    if (!decode(S, pos, v)) return false;
    if (v.type == T_MAP || v.type == T_ARRAY) {
        const uint64_t items = (uint64_t)v.n * (v.type == T_MAP ? 2 : 1);
        for (uint64_t k = 0; k < items; ++k)
            if (!skip_value(S, pos, depth + 1)) return false;
    }
    return true;
}

inline bool map_get(const Section& S, const Val& m, const char* key, Val& out, bool& found, int depth) {
    found = false;
    if (m.type != T_MAP) return true;
    const size_t kl = strlen(key);
    size_t pos = m.pos;
    for (uint32_t k = 0; k < m.n; ++k) {
        Val kv;
        if (!decode(S, pos, kv) || kv.type != T_UTF8) return false;
        const bool hit = !found && kv.n == kl && memcmp(kv.s, key, kl) == 0;
        if (hit) {
            size_t at = pos;
            if (!decode(S, at, out)) return false;
            found = true;  // (the first entry of a key; the walk goes on only to validate the map)
            return true;
        }
        if (!skip_value(S, pos, depth + 1)) return false;
    }
    return true;
}

// element idx of array a
inline bool array_get(const Section& S, const Val& a, uint32_t idx, Val& out) {
    if (a.type != T_ARRAY || idx >= a.n) return false;
    size_t pos = a.pos;
    for (uint32_t k = 0; k < idx; ++k)
        if (!skip_value(S, pos, 1)) return false;
    return decode(S, pos, out);
}

struct Db {
    std::vector<uint8_t> file;  // (data points into it: not resized after parse)
    uint32_t node_count = 0, record_size = 0, ip_version = 0;
    std::string database_type;
    Section data;  // the data section
    // the device tree image (lp_geoip.h) and, per record id, its data offset
    std::vector<uint64_t> tree;  // (u64 words: the header's two, then one per node, left | right << 32)
    std::vector<uint32_t> rec_off;
};

// record `side` (0 left, 1 right) of node n
inline uint32_t record(const Db& D, uint32_t n, int side) {
    const uint8_t* p = D.file.data() + (size_t)n * (D.record_size / 4);
    switch (D.record_size) {
    case 24: p += 3 * side; return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
    case 28:
        if (side == 0) return ((uint32_t)(p[3] >> 4) << 24) | ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
        return ((uint32_t)(p[3] & 15u) << 24) | ((uint32_t)p[4] << 16) | ((uint32_t)p[5] << 8) | p[6];
    default: p += 4 * side; return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    }
}

// Parse the bytes in D.file: metadata, sections, then the whole tree once --
// every record in range, no path longer than the address, every distinct data
// offset a dense record id -- into D.tree / D.rec_off.  false with why.
inline bool parse(Db& D, std::string& why) {
    static const uint8_t MARK[] = {0xab, 0xcd, 0xef, 'M', 'a', 'x', 'M', 'i', 'n', 'd', '.', 'c', 'o', 'm'};
    const size_t ML = sizeof MARK, n = D.file.size();
    size_t at = std::string::npos;
    for (size_t k = n >= ML ? n - ML + 1 : 0; k-- > 0;)
        if (memcmp(D.file.data() + k, MARK, ML) == 0) { at = k; break; }
    if (at == std::string::npos) { why = "no MaxMind DB metadata marker"; return false; }
    const Section M{D.file.data() + at + ML, n - at - ML};
    size_t pos = 0;
    Val meta;
    if (!decode(M, pos, meta) || meta.type != T_MAP) { why = "the metadata is not a map"; return false; }
    auto num = [&](const char* key, uint32_t& out) {
        Val v;
        bool found = false;
        if (!map_get(M, meta, key, v, found) || !found) return false;
        if (v.type != T_UINT16 && v.type != T_UINT32 && v.type != T_UINT64) return false;
        if (v.u > 0xFFFFFFFFull) return false;
        out = (uint32_t)v.u;
        return true;
    };
    if (!num("node_count", D.node_count) || !num("record_size", D.record_size) || !num("ip_version", D.ip_version)) {
        why = "the metadata lacks node_count, record_size or ip_version";
        return false;
    }
    Val ty;
    bool found = false;
    if (!map_get(M, meta, "database_type", ty, found) || !found || ty.type != T_UTF8) {
        why = "the metadata lacks database_type";
        return false;
    }
    D.database_type.assign((const char*)ty.s, ty.n);
    if (D.record_size != 24 && D.record_size != 28 && D.record_size != 32) { why = "record_size is not 24, 28 or 32"; return false; }
    if (D.ip_version != 4 && D.ip_version != 6) { why = "ip_version is not 4 or 6"; return false; }
    if (D.node_count == 0 || D.node_count >= 0x7FFFFFF0u) { why = "node_count out of range"; return false; }
    const uint64_t tree_bytes = (uint64_t)D.node_count * (D.record_size / 4);
    if (tree_bytes + 16 > at) { why = "the search tree does not fit the file"; return false; }
    D.data = Section{D.file.data() + tree_bytes + 16, at - (size_t)(tree_bytes + 16)};
    // the tree, once: depth[n] = the longest path that reaches node n (a node
    // may be shared: the IPv4 subtree's aliases); a longer path re-visits it
    const uint32_t N = D.node_count, bits = D.ip_version == 6 ? 128u : 32u;
    D.tree.assign(GEO_HDR / 2 + (size_t)N, 0);
    auto child_of = [&](uint32_t k, int side) { return (uint32_t)(D.tree[GEO_HDR / 2 + (size_t)k] >> (32 * side)); };
    D.rec_off.clear();
    std::unordered_map<uint32_t, uint32_t> id_of;
    for (uint32_t k = 0; k < N; ++k)
        for (int side = 0; side < 2; ++side) {
            const uint32_t r = record(D, k, side);
            uint32_t child;
            if (r < N) child = r;
            else if (r == N) child = GEO_NONE;
            else {
                const uint64_t off = (uint64_t)r - N - 16;
                if (r < N + 16 || off >= D.data.len) { why = "a record points outside the data section"; return false; }
                auto it = id_of.find((uint32_t)off);
                if (it == id_of.end()) {
                    it = id_of.emplace((uint32_t)off, (uint32_t)D.rec_off.size()).first;
                    D.rec_off.push_back((uint32_t)off);
                }
                child = GEO_REC | it->second;
            }
            D.tree[GEO_HDR / 2 + (size_t)k] |= (uint64_t)child << (32 * side);
        }
    std::vector<uint8_t> depth(N, 0);
    std::vector<uint8_t> seen(N, 0);
    std::vector<uint32_t> stack{0};
    seen[0] = 1;
    while (!stack.empty()) {
        const uint32_t k = stack.back();
        stack.pop_back();
        const uint32_t d = depth[k];
        if (d >= bits) { why = "a path of the search tree is longer than the address"; return false; }
        for (int side = 0; side < 2; ++side) {
            const uint32_t c = child_of(k, side);
            if (c >= N) continue;
            if (!seen[c] || depth[c] < d + 1) {
                seen[c] = 1;
                depth[c] = (uint8_t)(d + 1);
                stack.push_back(c);
            }
        }
    }
    // the IPv4 start: 96 zero bits from the root of an ip_version 6 tree, ended where the walk leaves the nodes
    uint32_t v4 = 0;
    if (D.ip_version == 6)
        for (int k = 0; k < 96 && v4 < N; ++k) v4 = child_of(v4, 0);
    D.tree[0] = (uint64_t)N | ((uint64_t)D.ip_version << 32);
    D.tree[1] = (uint64_t)v4 | ((uint64_t)D.rec_off.size() << 32);
    return true;
}

// Read path into D and parse it.  why: "<path> (<reason>)".
inline bool load(Db& D, const std::string& path, std::string& why) {
    FILE* f = path.empty() ? nullptr : fopen(path.c_str(), "rb");
    if (!f) { why = path + " (No such file or directory)"; return false; }
    D.file.clear();
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) D.file.insert(D.file.end(), buf, buf + got);
    fclose(f);
    std::string w;
    if (!parse(D, w)) { why = path + " (not a valid MaxMind DB file: " + w + ")"; return false; }
    return true;
}

// Double.toString(d): the shortest digits that read back as d, in Java's
// layout -- decimal notation for 1e-3 <= |d| < 1e7, else "d.dddE[-]n", always
// at least one digit after the point.
inline std::string java_double(double d) {
    if (d != d) return "NaN";
    if (d == 0) return std::signbit(d) ? "-0.0" : "0.0";
    if (d > 1.7976931348623157e308) return "Infinity";
    if (d < -1.7976931348623157e308) return "-Infinity";
    char b[40];
    int prec = 1;
    for (; prec < 17; ++prec) {
        snprintf(b, sizeof b, "%.*e", prec - 1, d);
        if (strtod(b, nullptr) == d) break;
    }
    snprintf(b, sizeof b, "%.*e", prec - 1, d);
    // b = [-]D[.DDD]e[+-]XX
    std::string s(b), digits;
    const bool neg = s[0] == '-';
    const size_t e = s.find('e');
    for (size_t k = neg ? 1 : 0; k < e; ++k)
        if (s[k] != '.') digits += s[k];
    const int exp = atoi(s.c_str() + e + 1);
    std::string out = neg ? "-" : "";
    if (exp >= -3 && exp < 7) {
        if (exp >= 0) {
            while ((int)digits.size() < exp + 1) digits += '0';
            out += digits.substr(0, (size_t)exp + 1) + ".";
            const std::string frac = digits.substr((size_t)exp + 1);
            out += frac.empty() ? "0" : frac;
        } else {
            out += "0." + std::string((size_t)(-exp - 1), '0') + digits;
        }
    } else {
        out += digits.substr(0, 1) + "." + (digits.size() > 1 ? digits.substr(1) : "0") + "E" + std::to_string(exp);
    }
    return out;
}

}  // namespace mmdb
}  // namespace lp
