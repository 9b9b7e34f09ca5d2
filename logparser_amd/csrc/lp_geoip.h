// The per-line work of the GeoIP dissectors (hp/dissectors/geoip/
// AbstractGeoIPDissector.java:93-110): the address text of an IP value to
// bits, then the walk of a MaxMind DB search tree.  __host__ __device__, as
// lp_value.h: k_geoip_lines (geoip.hip), the host replay's tests and the
// test-only emulation run this one source.
//
// The device images of a database (built once per handle by plan.cpp from
// lp_mmdb.h's reader, never by the kernels):
//   tree    u32 pairs read as one u64 each (the first word in the low half): a
//           header of GEO_HDR words (node count, ip_version; the IPv4 start,
//           record count), then one pair per node, left child first.  A
//           child is a node index (< node count), GEO_NONE (the file's
//           "record == node_count": not found) or GEO_REC | record id (a
//           data record; ids are dense, one per distinct data offset).
//           The 24 / 28 / 32-bit records of the file are unpacked on the host.
//   fields  one GeoField per (requested field, record id), field-major.
#pragma once
#include <stdint.h>

#include "lp_program.h"

#if defined(__HIP__)
#define LP_GEO_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define LP_GEO_HD inline
#endif

namespace lp {

constexpr uint32_t GEO_NONE = 0xFFFFFFFFu;
constexpr uint32_t GEO_REC = 0x80000000u;
constexpr int GEO_HDR = 4;           // node count, ip_version (4 / 6), IPv4 start (a child), record count
constexpr uint32_t GEO_NULL = 0xFFFFFFFFu;  // GeoField::off of a null value
constexpr int GEO_MAX_TEXT = 45;     // the longest address text decided here ("xxxx:" x 6 + a dotted quad)

// One requested field of one record.  STRING: off / len into the stage's byte
// pool.  LONG: v the value (two's complement).  DOUBLE: v the f64's bits and
// off / len its text as Double.toString prints it.  off == GEO_NULL: null.
struct GeoField {
    uint64_t v;
    uint32_t off, len;
};

// The outputs of the four classes in delivery order (GeoIPCountryDissector.java:
// 126-157, GeoIPCityDissector.java:205-280, GeoIPASNDissector.java:90-97,
// GeoIPISPDissector.java:93-100): field ids, bit k of ValStage::want.
enum : int32_t {
    GF_CONTINENT_NAME, GF_CONTINENT_CODE, GF_COUNTRY_NAME, GF_COUNTRY_ISO, GF_COUNTRY_CONFIDENCE, GF_COUNTRY_EU,
    GF_SUBDIVISION_NAME, GF_SUBDIVISION_ISO, GF_CITY_NAME, GF_CITY_CONFIDENCE, GF_CITY_GEONAMEID, GF_POSTAL_CODE,
    GF_POSTAL_CONFIDENCE, GF_LATITUDE, GF_LONGITUDE, GF_TIMEZONE, GF_ACCURACYRADIUS, GF_AVERAGEINCOME, GF_METROCODE,
    GF_POPULATIONDENSITY, GF_ASN_NUMBER, GF_ASN_ORGANIZATION, GF_ISP_NAME, GF_ISP_ORGANIZATION, GF_COUNT
};
enum : int32_t { GK_STRING = 0, GK_LONG = 1, GK_DOUBLE = 2 };  // TableSrc::c of a TC_GEOIP source
// a field's slot in its stage's field table: its rank among the wanted fields
LP_GEO_HD int geo_slot(uint32_t want, int field) {
    uint32_t m = want & ((1u << field) - 1u);
    int n = 0;
    for (; m; m &= m - 1) ++n;
    return n;
}

// The family ip_parse decided
enum : int { IPF_UNDECIDED = 0, IPF_V4 = 4, IPF_V6 = 6 };

// 128 bits as two u64, shifted left by 0..128 bits
LP_GEO_HD void geo_shl128(uint64_t& hi, uint64_t& lo, uint32_t s) {
    if (s >= 128) { hi = lo = 0; }
    else if (s >= 64) { hi = s == 64 ? lo : lo << (s - 64); lo = 0; }
    else if (s) { hi = (hi << s) | (lo >> (64 - s)); lo <<= s; }
}

// InetAddress.getByName(text) for the texts whose answer needs neither DNS
// nor a legacy form: the decided subset.  w: the text's n bytes, byte k in
// bits 8 (k & 3).. of w[k >> 2] (the bytes past n are not read as text).
//   dotted quad      four decimal parts 0-255 of 1-3 digits, no leading zero
//                    on a multi-digit part                          -> IPF_V4
//   RFC 4291 text    eight groups of 1-4 hex digits, or fewer with exactly
//                    one "::"; the last two groups may be written as such a
//                    dotted quad                                    -> IPF_V6
//   ... whose bytes are IPv4-mapped (::ffff:a.b.c.d): the JDK returns an
//                    Inet4Address (IPAddressUtil.convertFromIPv4MappedAddress) -> IPF_V4
// a[0] holds the 32 bits of an IPv4 address (a[1..3] = 0), a[0..3] the 128
// bits of an IPv6 address, most significant word first.  Anything else --
// host names, "1.2.3", "01.2.3.4", brackets, a scope id, more than 45 bytes --
// is IPF_UNDECIDED.  One pass, a constant trip count: with w in registers the
// loop unrolls into straight-line code (no indexed register access).
LP_GEO_HD int ip_parse_words(const uint32_t (&w)[12], uint32_t n, uint32_t a[4]) {
    a[0] = a[1] = a[2] = a[3] = 0;
    if (n == 0 || n > (uint32_t)GEO_MAX_TEXT) return IPF_UNDECIDED;
    bool bad = false, quad = false, colon = false, gap = false, alldec = true, lead0 = false;
    // last: 0 start, 1 a digit, 2 a single ':', 3 "::", 4 the '.' of a quad
    uint32_t last = 0, cur = 0, dec = 0, nd = 0, ng = 0, nH = 0, q = 0, nq = 0;
    uint64_t hi = 0, lo = 0, Hhi = 0, Hlo = 0;
    auto push = [&](uint32_t g) {  // one 16-bit group
        hi = (hi << 16) | (lo >> 48);
        lo = (lo << 16) | g;
        ++ng;
        bad = bad || nH + ng > 8u;
    };
    LP_UNROLL
    for (uint32_t k = 0; k < (uint32_t)GEO_MAX_TEXT; ++k) {
        if (k >= n) continue;
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
        const uint32_t d = c - '0', x = (c | 32u) - 'a';
        if (quad) {
            if (d < 10u) {
                if (nd == 0) lead0 = d == 0;
                else bad = bad || lead0;
                dec = dec * 10 + d;
                ++nd;
                bad = bad || nd > 3u;
                last = 1;
            } else if (c == '.' && last == 1) {
                bad = bad || dec > 255u || nq >= 3u;
                q = (q << 8) | (dec & 255u);
                ++nq;
                dec = nd = 0;
                last = 4;
            } else {
                bad = true;
            }
        } else if (d < 10u || x < 6u) {
            bad = bad || (last == 2 && ng == 0 && !gap);  // ":1": a leading single ':'
            if (nd == 0) { cur = dec = 0; alldec = true; lead0 = d == 0; }
            cur = (cur << 4) | (d < 10u ? d : x + 10u);
            if (d < 10u) dec = dec * 10 + d;
            else alldec = false;
            ++nd;
            bad = bad || nd > 4u;
            last = 1;
        } else if (c == ':') {
            colon = true;
            if (last == 1) { push(cur); nd = 0; last = 2; }
            else if (last == 0) last = 2;
            else if (last == 2 && !gap) {  // "::": the groups so far are the head
                gap = true;
                nH = ng;
                Hhi = hi;
                Hlo = lo;
                hi = lo = 0;
                ng = 0;
                last = 3;
            } else {
                bad = true;  // ":::", a second "::"
            }
        } else if (c == '.' && last == 1 && alldec && nd <= 3u) {
            // the last two groups as a dotted quad: the digits read so far are its first part
            bad = bad || (nd > 1u && lead0) || dec > 255u;
            quad = true;
            q = dec & 255u;
            nq = 1;
            dec = nd = 0;
            last = 4;
        } else {
            bad = true;
        }
    }
    if (quad) {
        bad = bad || last != 1 || nq != 3u || dec > 255u;
        q = (q << 8) | (dec & 255u);
        if (!colon) {
            if (bad) return IPF_UNDECIDED;
            a[0] = q;
            return IPF_V4;
        }
        push(q >> 16);
        push(q & 0xFFFFu);
    } else {
        if (last == 1) push(cur);
        bad = bad || !colon || last == 2;  // no ':' at all (a name, a number), a trailing single ':'
    }
    bad = bad || (gap ? nH + ng > 7u : ng != 8u);
    if (bad) return IPF_UNDECIDED;
    if (gap) {
        geo_shl128(Hhi, Hlo, 16u * (8u - nH));
        hi |= Hhi;
        lo |= Hlo;
    }
    if (hi == 0 && (lo >> 32) == 0xFFFFull) {  // IPv4-mapped: looked up as IPv4
        a[0] = (uint32_t)lo;
        return IPF_V4;
    }
    a[0] = (uint32_t)(hi >> 32);
    a[1] = (uint32_t)hi;
    a[2] = (uint32_t)(lo >> 32);
    a[3] = (uint32_t)lo;
    return IPF_V6;
}

// The kernel's register-staged token: x holds the four aligned 16-byte blocks
// around the text (a block without text bytes: zeros), the text starts at
// byte m (0..15) of x.  w: the text's bytes from byte 0 on (12 words; at most
// 45 text bytes), by a word shift and a funnel shift -- constant indices only.
LP_GEO_HD void ip_align_words(const uint32_t (&x)[16], uint32_t m, uint32_t (&w)[12]) {
    // a barrel shifter over whole words -- by one word, then by two -- with bit masks: written as
    // a choice between x[q] .. x[q + 3] the device compiler keeps x in scratch and indexes it by m
    uint32_t m1 = 0u - ((m >> 2) & 1u), m2 = 0u - (m >> 3);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(m1), "+v"(m2));  // (opaque: all ones or zero)
#endif
    const uint32_t mb = (m & 3u) * 8u;
    uint32_t t[15], y[13];
    LP_UNROLL
    for (int q = 0; q < 15; ++q) t[q] = x[q] ^ ((x[q] ^ x[q + 1]) & m1);
    LP_UNROLL
    for (int q = 0; q < 13; ++q) y[q] = t[q] ^ ((t[q] ^ t[q + 2]) & m2);
    LP_UNROLL
    for (int q = 0; q < 12; ++q) w[q] = mb ? (y[q] >> mb) | (y[q + 1] << (32u - mb)) : y[q];
}

// ip_parse_words on the bytes [p, p + n): reads only those, byte by byte
// (host code, and the emulation of the kernel's register-staged load)
template <class In>
LP_GEO_HD int ip_parse(In p, uint32_t n, uint32_t a[4]) {
    uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n <= (uint32_t)GEO_MAX_TEXT)
        for (uint32_t k = 0; k < n; ++k) w[k >> 2] |= (uint32_t)(uint8_t)p[k] << (8 * (k & 3));
    return ip_parse_words(w, n, a);
}

// Reader.get(InetAddress) of maxmind-db on a tree image: the record id + 1 of
// the address a (ip_parse's words, family fam), 0 when it is not in the
// tree.  An IPv4 address in an ip_version 6 tree starts at the header's IPv4
// start, the node 96 zero bits lead to -- itself "not found" or a data record
// when the walk left the nodes before.  One 8-byte load per level; the loop
// ends at the first leaf.  img: the image as u64 words.  fam must be IPF_V4, or IPF_V6 with an ip_version 6
// tree (the caller sends an IPv6 address against an ip_version 4 tree to
// FALLBACK).  The host validated the image: every child is in range and no
// path is longer than the address.
template <class Img>
LP_GEO_HD uint32_t geo_walk(Img img, const uint32_t a[4], int fam) {
    const uint32_t nodes = (uint32_t)img[0];
    uint32_t cur = fam == IPF_V4 ? (uint32_t)img[1] : 0u;
    uint32_t a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
    const int bits = fam == IPF_V4 ? 32 : 128;
    for (int k = 0; k < bits && cur < nodes; ++k) {
        const uint64_t pair = img[GEO_HDR / 2 + (size_t)cur];
        cur = (a0 >> 31) ? (uint32_t)(pair >> 32) : (uint32_t)pair;
        a0 = (a0 << 1) | (a1 >> 31);
        a1 = (a1 << 1) | (a2 >> 31);
        a2 = (a2 << 1) | (a3 >> 31);
        a3 <<= 1;
    }
    if (cur == GEO_NONE || !(cur & GEO_REC)) return 0;
    return (cur & ~GEO_REC) + 1u;
}

// One GeoIP stage of one line once its text is parsed: the record id + 1, 0
// for an address that is not in the tree, -1 when the reference owns the line
// (FALLBACK): a text outside the decided subset -- getByName would ask DNS or
// accept a legacy form -- or an IPv6 address against an ip_version 4 tree.
template <class Img>
LP_GEO_HD int64_t geo_resolve(Img img, const uint32_t a[4], int fam) {
    if (fam == IPF_UNDECIDED || (fam == IPF_V6 && (uint32_t)(img[0] >> 32) != 6u)) return -1;
    return (int64_t)geo_walk(img, a, fam);
}
// ... of the value [p, p + n) (n > 0), read byte by byte
template <class In, class Img>
LP_GEO_HD int64_t geo_lookup(In p, uint32_t n, Img img) {
    uint32_t a[4];
    const int fam = ip_parse(p, n, a);
    return geo_resolve(img, a, fam);
}

}  // namespace lp
