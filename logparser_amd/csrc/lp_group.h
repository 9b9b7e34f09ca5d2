// The core of the grouped aggregates (lp_result_group, group.hip): the hash of
// a row's key tuple, the accumulator words of a group, what a row contributes
// to each of them, and how two partial results merge.  Compiles for the device
// (group.hip) and for the host (capi.cpp's layout; tests/emu/group_emu.cpp runs
// it from several threads under the sanitizers); the atomics come through a
// small shim (GroupAtDevice / GroupAtHost), as lp_dict.h's do.
//
// Grouping is lp_dict.h's insert on a 64-bit hash of the whole key tuple: a
// row stores its hash, then claims or finds its class's slot; same(r) looks at
// row r's stored hash first.  That word is written by the lane of row r in the
// same launch, and nothing orders it against r's appearance in a slot (the
// insert's atomics are relaxed, the XCDs' L2s private).  So the word validates
// itself: the array is zeroed before the launch, a stored hash carries
// GROUP_HASH_SET, and one 8-byte atomic store / load moves it.  A reader that
// still sees 0 learns nothing and compares the keys in full -- values an
// earlier launch wrote, as the dictionary's same(r) reads -- so a late hash
// costs time, never the result.  No fence, no wait.
//
// A group's accumulators are 64-bit words, every one an order-independent
// fold -- wrapping add, min or max -- so that any split of the rows into
// partial results (a block's LDS copy, a wave's peeled group, a lane) merges
// to the same bits:
//   word 0             the group's rows
//   word 1 + m         the rows on which distinct measure m is not null: the
//                      value of its COUNT, the has-value test of its SUM / MIN / MAX
//   then one word per SUM / MIN / MAX aggregate, in the aggregates' order
// A word starts at its fold's identity; a contribution equal to the identity
// is never issued (a null measure, a block that did not touch the group).
#pragma once
#include <stdint.h>

#include "lp_dict.h"

namespace lp {

constexpr int GROUP_MAX_KEYS = 4, GROUP_MAX_AGGS = 8;
constexpr int GROUP_MAX_WORDS = 1 + 2 * GROUP_MAX_AGGS;
// LP_AGG_*; a word's kind is the same number (GA_COUNT_ROWS: word 0, GA_COUNT: a measure's non-null count)
enum : int32_t { GA_COUNT_ROWS = 0, GA_COUNT, GA_SUM, GA_MIN, GA_MAX };
// the default LDS budget of k_group_agg's privatised regime, in words, and the direct regime's peel rounds
// 
constexpr int GROUP_LDS_WORDS = 4096, GROUP_LDS_WORDS_MAX = 8192;
constexpr int GROUP_PEEL_ROUNDS = 2, GROUP_PEEL_MAX = 4;

// ---- the key tuple's hash: per key a tag (0 null, else its kind), then the
// int64, or dict_hash of the bytes' words; dict_mix throughout
constexpr uint64_t GROUP_SEED = 0x13198A2E03707344ull;
LP_DICT_HD uint64_t group_hash_null(uint64_t h) { return dict_mix(h, 0); }
LP_DICT_HD uint64_t group_hash_long(uint64_t h, int64_t l) { return dict_mix(dict_mix(h, 2), (uint64_t)l); }
template <class Word>
LP_DICT_HD uint64_t group_hash_bytes(uint64_t h, uint32_t n, Word word) {
    return dict_mix(dict_mix(h, 1), dict_hash(n, word));
}
// the stored hash: finalised; bits 1..32 (LP_OPT_DICT_HASH_BITS): only that
// many low bits survive, in the home slot (dict_home takes the same bits) and
// in the stored word, so distinct tuples meet in the probe and in the full compare
constexpr uint64_t GROUP_HASH_SET = 1ull << 63;  // in a stored word (its bit 63 is not compared)
LP_DICT_HD uint64_t group_hash_end(uint64_t h, int bits) {
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return bits > 0 && bits < 64 ? h & ((1ull << bits) - 1) : h;
}

// may row r, whose stored word is `stored`, have the hash h?  (0: not seen yet)
LP_DICT_HD bool group_hash_may_equal(uint64_t stored, uint64_t h) { return stored == 0 || stored == (h | GROUP_HASH_SET); }

// ---- the accumulator words
struct GroupAccs {
    int32_t n_aggs, n_meas, n_words, pad;
    int32_t op[GROUP_MAX_AGGS];     // GA_*
    int32_t meas[GROUP_MAX_AGGS];   // the aggregate's distinct measure (-1: COUNT_ROWS)
    int32_t word[GROUP_MAX_AGGS];   // the word its value is read from
    int32_t wkind[GROUP_MAX_WORDS]; // each word's GA_* kind
    int32_t wmeas[GROUP_MAX_WORDS]; // ... and measure (-1: word 0)
};

// ops / meas of n_aggs aggregates over n_meas distinct measures
inline GroupAccs group_accs(int n_aggs, const int32_t* op, const int32_t* meas, int n_meas) {
    GroupAccs A{};
    A.n_aggs = n_aggs;
    A.n_meas = n_meas;
    A.wkind[0] = GA_COUNT_ROWS;
    A.wmeas[0] = -1;
    for (int m = 0; m < n_meas; ++m) {
        A.wkind[1 + m] = GA_COUNT;
        A.wmeas[1 + m] = m;
    }
    int w = 1 + n_meas;
    for (int a = 0; a < n_aggs; ++a) {
        A.op[a] = op[a];
        A.meas[a] = op[a] == GA_COUNT_ROWS ? -1 : meas[a];
        if (op[a] == GA_COUNT_ROWS) A.word[a] = 0;
        else if (op[a] == GA_COUNT) A.word[a] = 1 + meas[a];
        else {
            A.wkind[w] = op[a];
            A.wmeas[w] = meas[a];
            A.word[a] = w++;
        }
    }
    A.n_words = w;
    return A;
}

LP_DICT_HD int64_t group_identity(int32_t kind) {
    return kind == GA_MIN ? INT64_MAX : kind == GA_MAX ? INT64_MIN : 0;
}
// two partial results of a word of `kind` (the sum wraps: Java's long +)
LP_DICT_HD int64_t group_merge(int32_t kind, int64_t a, int64_t b) {
    if (kind == GA_MIN) return a < b ? a : b;
    if (kind == GA_MAX) return a > b ? a : b;
    return (int64_t)((uint64_t)a + (uint64_t)b);
}
// what a row whose measure (of the word) is ok / x gives a word of `kind`
LP_DICT_HD int64_t group_contrib(int32_t kind, bool ok, int64_t x) {
    if (kind == GA_COUNT_ROWS) return 1;
    if (kind == GA_COUNT) return ok ? 1 : 0;
    return ok ? x : group_identity(kind);
}
// v folded into *word, unless it is the identity: what a lane does to a
// block's LDS copy or to the global word, and a block's flush of its copy
template <class At, class P>
LP_DICT_HD void group_fold(P word, int32_t kind, int64_t v) {
    if (v == group_identity(kind)) return;
    if (kind == GA_MIN) At::fetch_min(word, v);
    else if (kind == GA_MAX) At::fetch_max(word, v);
    else At::fetch_add(word, v);
}
// aggregate a's value and validity out of its group's words
LP_DICT_HD int64_t group_value(const GroupAccs& A, int a, const int64_t* w, uint8_t& valid) {
    valid = A.op[a] <= GA_COUNT || w[1 + A.meas[a]] != 0;
    return valid ? w[A.word[a]] : 0;
}
// the regime of a call: the privatised one when every group's words fit the budget
LP_DICT_HD bool group_privatised(int64_t n_groups, int n_words, int64_t budget) {
    return n_groups * (int64_t)n_words <= budget;
}

#if defined(__HIPCC__)
// SCOPE: agent for the global words (the XCDs do not share an L2), workgroup
// for a block's LDS copy
template <int SCOPE>
struct GroupAtDevice {
    template <class P>
    static __device__ __forceinline__ void store_hash(P p, uint64_t v) {
        __hip_atomic_store((uint64_t*)p, v | GROUP_HASH_SET, __ATOMIC_RELAXED, SCOPE);
    }
    template <class P>
    static __device__ __forceinline__ uint64_t load_hash(P p) {
        return __hip_atomic_load((const uint64_t*)p, __ATOMIC_RELAXED, SCOPE);
    }
    template <class P>
    static __device__ __forceinline__ void fetch_add(P p, int64_t v) {
        __hip_atomic_fetch_add((uint64_t*)p, (uint64_t)v, __ATOMIC_RELAXED, SCOPE);
    }
    template <class P>
    static __device__ __forceinline__ void fetch_min(P p, int64_t v) {
        __hip_atomic_fetch_min((int64_t*)p, v, __ATOMIC_RELAXED, SCOPE);
    }
    template <class P>
    static __device__ __forceinline__ void fetch_max(P p, int64_t v) {
        __hip_atomic_fetch_max((int64_t*)p, v, __ATOMIC_RELAXED, SCOPE);
    }
};
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
struct GroupAtHost {
    static inline void store_hash(uint64_t* p, uint64_t v) {
        __atomic_store_n(p, v | GROUP_HASH_SET, __ATOMIC_RELAXED);
    }
    static inline uint64_t load_hash(const uint64_t* p) {
        return __atomic_load_n(p, __ATOMIC_RELAXED);
    }
    static inline void fetch_add(int64_t* p, int64_t v) { __atomic_fetch_add((uint64_t*)p, (uint64_t)v, __ATOMIC_RELAXED); }
    static inline void fetch_min(int64_t* p, int64_t v) {
        int64_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (cur > v && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
    static inline void fetch_max(int64_t* p, int64_t v) {
        int64_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (cur < v && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
};
#endif

}  // namespace lp
