// The pure value conversions of the typed table (table_value.h, table.hip,
// dict.hip): the length and the text of a long (Long.toString), Long.parseLong
// and Double.parseDouble of "I.F".  Compiles for the device (the table
// kernels, through table_value.h) and for the host (tests/emu/value_emu.cpp
// checks it against strtoll / strtod / snprintf under the sanitizers).
// Internal linkage: each unit that includes it gets its own copy.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LP_VAL_HD __host__ __device__
#define LP_VAL_INLINE __host__ __device__ __forceinline__
#else
#include <cmath>
#define LP_VAL_HD
#define LP_VAL_INLINE inline
#endif
#ifndef LP_G  // (lp_program.h: the kernel units' global-memory pointers)
#define LP_G
#endif

namespace lp {

static LP_VAL_INLINE uint32_t digits(int64_t l) {
    uint64_t u = l < 0 ? 0 - (uint64_t)l : (uint64_t)l;
    uint32_t n = 1;
    while (u >= 10) { u /= 10; ++n; }
    return n + (l < 0 ? 1u : 0u);
}

// Out: a byte pointer of any address space
template <class Out>
static LP_VAL_INLINE void write_long(Out d, int64_t l, uint32_t n) {  // n = digits(l)
    uint64_t u = l < 0 ? 0 - (uint64_t)l : (uint64_t)l;
    uint32_t k = n;
    do {
        d[--k] = (uint8_t)('0' + u % 10);
        u /= 10;
    } while (u);
    if (l < 0) d[0] = '-';
}

// Long.parseLong (the host table's java_parse_long)
static LP_VAL_HD bool parse_long(const LP_G uint8_t* p, uint32_t n, bool amp, int64_t& out) {
    if (amp || n == 0) return false;
    uint32_t k = 0;
    bool neg = false;
    if (p[0] == '-' || p[0] == '+') { neg = p[0] == '-'; k = 1; }
    if (k == n) return false;
    uint64_t v = 0;
    for (; k < n; ++k) {
        const uint32_t d = p[k] - '0';
        if (d > 9) return false;
        if (v > (0x8000000000000000ull - d) / 10) return false;  // past 2^63
        v = v * 10 + d;
    }
    if (!neg && v == 0x8000000000000000ull) return false;
    out = neg ? (int64_t)(0 - v) : (int64_t)v;
    return true;
}

// Double.parseDouble of "I.F" (digits '.' digits, each at most 18 digits:
// a SECOND_MILLIS upstream list item, UpstreamModule's element kind):
// correctly rounded, as Java's parse (IEEE round half to even).  S = I *
// 10^f + F and the value is S / 10^f: exact by one IEEE division when S <
// 2^53 and f <= 22 (both operands exact); else the quotient's 54-55
// leading bits by binary long division in 128-bit integers (S < 2^120),
// rounded with the remainder as the sticky bit.
static LP_VAL_HD double decimal_to_double(const LP_G uint8_t* p, uint32_t n) {
    typedef unsigned __int128 u128;
    uint64_t I = 0, F = 0;
    uint32_t q = 0;
    int f = 0;
    for (; q < n && p[q] != '.'; ++q) I = I * 10u + (p[q] - '0');
    for (++q; q < n; ++q, ++f) F = F * 10u + (p[q] - '0');
    u128 D = 1;
    for (int k = 0; k < f; ++k) D *= 10u;
    const u128 S = (u128)I * D + F;
    if (S == 0) return 0.0;
    if (S < ((u128)1 << 53) && f <= 22) return (double)(uint64_t)S / (double)(uint64_t)D;
    auto bitlen = [](u128 x) {
        const uint64_t hi = (uint64_t)(x >> 64), lo = (uint64_t)x;
        return hi ? 128 - __builtin_clzll(hi) : lo ? 64 - __builtin_clzll(lo) : 0;
    };
    const int k = 54 - (bitlen(S) - bitlen(D));  // S * 2^k / D in [2^53, 2^55)
    u128 N = S, Dn = D;
    if (k >= 0) N <<= k;
    else Dn <<= -k;
    uint64_t quo = 0;
    for (int b = 55; b >= 0; --b) {
        const u128 t = Dn << b;
        if (N >= t) {
            N -= t;
            quo |= 1ull << b;
        }
    }
    const int shift = quo >= (1ull << 54) ? 2 : 1;  // keep 53 significant bits
    const uint64_t half = 1ull << (shift - 1), r = quo & ((1ull << shift) - 1);
    uint64_t m = quo >> shift;
    if (r > half || (r == half && (N != 0 || (m & 1u)))) ++m;
    return ldexp((double)m, shift - k);
}

// ScreenResolutionDissector.dissect (hp/dissectors/ScreenResolutionDissector.java:56-63)
// on the value [p, p + n): fieldValue.split("x") -- the separator is always
// "x": the instance that dissects is getNewInstance()'s (core/Parser.java:424-428,
// core/Dissector.java:135-145), which never sees the registered settings.
// String.split drops trailing empty strings and keeps leading and inner ones.
// Returns the number of parts, -1 when the value holds no 'x' (contains() is
// false: nothing is delivered); parts[0] = [0, w_len) when there is one,
// parts[1] = [h_off, h_off + h_len) when there are two.  Reads only p[0, n),
// byte by byte.  In: a byte pointer of any address space.
template <class In>
static LP_VAL_INLINE int screen_split(In p, uint32_t n, uint32_t& w_len, uint32_t& h_off, uint32_t& h_len) {
    uint32_t e = n;
    while (e > 0 && p[e - 1] == 'x') --e;  // the trailing empty strings
    uint32_t cnt = 0, x0 = e, x1 = e;      // the 'x' of [0, e): how many, the first two
    for (uint32_t q = 0; q < e; ++q) {
        if (p[q] != 'x') continue;
        if (cnt == 0) x0 = q;
        else if (cnt == 1) x1 = q;
        ++cnt;
    }
    w_len = x0;
    h_off = cnt ? x0 + 1 : e;
    h_len = cnt ? x1 - (x0 + 1) : 0;
    if (e == n && cnt == 0) return -1;
    return e == 0 ? 0 : (int)cnt + 1;
}

// ModUniqueIdDissector.decode (hp/dissectors/ModUniqueIdDissector.java:149-238)
// on the value [p, p + n): false (nothing is delivered) unless it is exactly 24
// letters of [A-Za-z0-9_-] -- length() != 24 is null (:150-152); '+' and '/'
// become '@' (:171-178), and commons-codec 1.11's Base64.decodeBase64 skips
// every byte outside its two alphabets and stops at '=', so any other byte
// leaves fewer than 24 sextets, fewer than 18 bytes, null (:195-197).  The
// sextets: A-Z 0-25, a-z 26-51, 0-9 52-61, and the URL-safe '-' 62, '_' 63
// (the codec decodes both alphabets).  The 18 bytes, big-endian and unsigned
// (:207-235): f[0] = u32(b0..3) the seconds (epoch = f[0] * 1000), f[1] =
// u32(b4..7) the address, f[2] = u32(b8..11) processid, f[3] = u16(b12..13)
// counter, f[4] = u32(b14..17) threadindex.  Reads only p[0, 24), byte by byte.
template <class In>
static LP_VAL_INLINE bool unique_id_decode(In p, uint32_t n, uint32_t f[5]) {
    if (n != 24) return false;
    uint32_t g[6];
    bool ok = true;
    for (int k = 0; k < 6; ++k) {
        uint32_t w = 0;
        for (int q = 0; q < 4; ++q) {
            const uint32_t c = p[4 * k + q];
            uint32_t s = 64;
            if (c - 'A' < 26u) s = c - 'A';
            else if (c - 'a' < 26u) s = c - 'a' + 26u;
            else if (c - '0' < 10u) s = c - '0' + 52u;
            else if (c == '-') s = 62;
            else if (c == '_') s = 63;
            ok = ok && s < 64u;
            w = (w << 6) | (s & 63u);
        }
        g[k] = w;  // three bytes
    }
    f[0] = (g[0] << 8) | (g[1] >> 16);
    f[1] = ((g[1] & 0xFFFFu) << 16) | (g[2] >> 8);
    f[2] = ((g[2] & 0xFFu) << 24) | g[3];
    f[3] = g[4] >> 8;
    f[4] = ((g[4] & 0xFFu) << 24) | g[5];
    return ok;
}

// the address of a mod_unique_id as "b4.b5.b6.b7" in unsigned decimals
// (ModUniqueIdDissector.java:219-222) into b (at most 15 bytes): its length
template <class Out>
static LP_VAL_INLINE uint32_t unique_id_ip(uint32_t ip, Out b) {
    uint32_t n = 0;
    for (int k = 3; k >= 0; --k) {
        const uint32_t x = (ip >> (8 * k)) & 0xFFu;
        if (k != 3) b[n++] = '.';
        if (x >= 100) b[n++] = (char)('0' + x / 100);
        if (x >= 10) b[n++] = (char)('0' + (x / 10) % 10);
        b[n++] = (char)('0' + x % 10);
    }
    return n;
}

}  // namespace lp
