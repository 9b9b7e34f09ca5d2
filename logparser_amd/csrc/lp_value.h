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

}  // namespace lp
