// The pure term rules of lp_result_select_where (include/logparser_amd.h): the
// LONG comparisons, the bytewise STRING operations and the fold of the terms'
// outcomes into a line's.  Compiles for the device (where.hip's k_where_eval)
// and for the host (capi.cpp's host-copy path; tests/emu/pred_emu.cpp checks
// it against memcmp / memmem / std::string under the sanitizers): the rules
// exist in this one copy.  Internal linkage: each unit that includes it gets
// its own.
//
// Two-valued logic: a comparison with a null value is false, IS_NULL is true
// exactly on null, and NEGATE flips the term's outcome after that rule.
//
// Read bound: an operation reads value bytes only through a view's at(k), k <
// len().  PredBytes reads them one by one; PredWords reads the aligned 4-byte
// word that holds the byte (and keeps it for the next three), so never a byte
// outside the aligned words that hold the value's bytes.  The operand is read
// byte by byte, [0, m).
#pragma once
#include <stdint.h>

#include "lp_value.h"  // LP_VAL_HD, LP_VAL_INLINE, LP_G

namespace lp {

// the ops of include/logparser_amd.h (LP_WHERE_*)
enum : int32_t {
    PRED_IS_NULL = 0, PRED_EQ, PRED_LT, PRED_LE, PRED_GT, PRED_GE, PRED_BETWEEN, PRED_PREFIX, PRED_SUFFIX, PRED_CONTAINS,
    PRED_N_OPS,
    PRED_NEGATE = 0x100,
};
constexpr int PRED_MAX_TERMS = 8;
constexpr int PRED_MAX_STR = 255;

// does the op (NEGATE or-ed in or not) exist for a column of kind (1 STRING, 2 LONG)?
static LP_VAL_INLINE bool pred_op_ok(int32_t op, int kind) {
    if (op & ~(PRED_NEGATE | 0xFF)) return false;
    const int32_t b = op & 0xFF;
    if (b == PRED_IS_NULL || b == PRED_EQ) return kind == 1 || kind == 2;
    if (b >= PRED_LT && b <= PRED_BETWEEN) return kind == 2;
    return b >= PRED_PREFIX && b <= PRED_CONTAINS && kind == 1;
}

// a non-null long against the operands (op without NEGATE)
static LP_VAL_INLINE bool pred_long(int32_t op, int64_t v, int64_t lo, int64_t hi) {
    switch (op) {
    case PRED_EQ: return v == lo;
    case PRED_LT: return v < lo;
    case PRED_LE: return v <= lo;
    case PRED_GT: return v > lo;
    case PRED_GE: return v >= lo;
    case PRED_BETWEEN: return lo <= v && v <= hi;  // (lo > hi: nothing)
    default: return false;
    }
}

// ---- value views: len() bytes, at(k) the k-th.  amp: a virtual '&' in front
// of the n bytes at p (a raw query string, lp_program.h ref_amp).
template <class P>  // a byte pointer of any address space
struct PredBytes {
    P p;
    uint32_t n;
    bool amp;
    LP_VAL_INLINE uint32_t len() const { return n + (amp ? 1u : 0u); }
    LP_VAL_INLINE uint8_t at(uint32_t k) {
        if (amp) {
            if (k == 0) return (uint8_t)'&';
            --k;
        }
        return p[k];
    }
};
// the same bytes through their aligned 4-byte words (W: a pointer to uint32_t
// of p's address space); the last word read serves its other bytes
template <class P, class W>
struct PredWords {
    P p;
    uint32_t n;
    bool amp;
    uintptr_t have = 0;  // the address of the word in w (0: none)
    uint32_t w = 0;
    LP_VAL_INLINE uint32_t len() const { return n + (amp ? 1u : 0u); }
    LP_VAL_INLINE uint8_t at(uint32_t k) {
        if (amp) {
            if (k == 0) return (uint8_t)'&';
            --k;
        }
        const uintptr_t a = (uintptr_t)(p + k), wa = a & ~(uintptr_t)3;
        if (wa != have) {
            w = *(W)(p + k - (a & 3u));
            have = wa;
        }
        return (uint8_t)(w >> (8 * (a & 3u)));  // (little-endian)
    }
};
// up to 20 local bytes (a formatted long, date, time, month name, binary IP)
struct PredLocal {
    const char* b;
    uint32_t n;
    LP_VAL_INLINE uint32_t len() const { return n; }
    LP_VAL_INLINE uint8_t at(uint32_t k) { return (uint8_t)b[k]; }
};

// the m operand bytes at o against the value's bytes [s, s + m) (s + m <= len())
template <class V, class O>
static LP_VAL_INLINE bool pred_match_at(V& v, uint32_t s, O o, uint32_t m) {
    for (uint32_t k = 0; k < m; ++k)
        if (v.at(s + k) != o[k]) return false;
    return true;
}

// a non-null byte string against the operand o[0, m) (op without NEGATE).  An
// empty operand: PREFIX / SUFFIX / CONTAINS hold on every value, EQ on the
// empty one.  CONTAINS is the plain search: a first-byte test, then a compare.
template <class V, class O>
static LP_VAL_INLINE bool pred_bytes(int32_t op, V& v, O o, uint32_t m) {
    const uint32_t n = v.len();
    switch (op) {
    case PRED_EQ: return n == m && pred_match_at(v, 0u, o, m);
    case PRED_PREFIX: return n >= m && pred_match_at(v, 0u, o, m);
    case PRED_SUFFIX: return n >= m && pred_match_at(v, n - m, o, m);
    case PRED_CONTAINS: {
        if (m == 0) return true;
        if (n < m) return false;
        const uint8_t o0 = o[0];
        for (uint32_t s = 0; s + m <= n; ++s)
            if (v.at(s) == o0 && pred_match_at(v, s + 1, o + 1, m - 1)) return true;
        return false;
    }
    default: return false;
    }
}

// a term's outcome from its value's: null -- IS_NULL true, every comparison
// false; then NEGATE
static LP_VAL_INLINE bool pred_outcome(int32_t op, bool null, bool holds) {
    const bool r = (op & 0xFF) == PRED_IS_NULL ? null : (!null && holds);
    return r != ((op & PRED_NEGATE) != 0);
}
static LP_VAL_INLINE bool pred_term_long(int32_t op, bool null, int64_t v, int64_t lo, int64_t hi) {
    return pred_outcome(op, null, !null && pred_long(op & 0xFF, v, lo, hi));
}
template <class V, class O>
static LP_VAL_INLINE bool pred_term_bytes(int32_t op, bool null, V& v, O o, uint32_t m) {
    return pred_outcome(op, null, !null && (op & 0xFF) != PRED_IS_NULL && pred_bytes(op & 0xFF, v, o, m));
}

// ---- the fold: AND over the groups of (OR over the group's terms); no terms:
// true.  In the terms' order: pred_fold_group(f, t, group) before term t, then
// -- only when pred_fold_wants(f): the line is still undecided by this term --
// pred_fold_term(f, outcome); at the end pred_fold_result(f, n_terms).
struct PredFold {
    bool live = true;  // every finished group held
    bool any = false;  // a term of the current group held
    int32_t group = 0;
};
static LP_VAL_INLINE void pred_fold_group(PredFold& f, int t, int32_t group) {
    if (t > 0 && group != f.group) {
        f.live = f.live && f.any;
        f.any = false;
    }
    f.group = group;
}
static LP_VAL_INLINE bool pred_fold_wants(const PredFold& f) { return f.live && !f.any; }
static LP_VAL_INLINE void pred_fold_term(PredFold& f, bool outcome) { f.any = f.any || outcome; }
static LP_VAL_INLINE bool pred_fold_result(const PredFold& f, int n_terms) { return f.live && (n_terms == 0 || f.any); }

}  // namespace lp
