// The core of the dictionary-encoded STRING columns (lp_result_table_dict,
// dict.hip): the hash of a value and the lock-free insert into an
// open-addressing table of row numbers.  Compiles for the device (dict.hip)
// and for the host (tests/emu/dict_emu.cpp runs it from several threads under
// the sanitizers); the atomics come through a small shim (DictAtDevice /
// DictAtHost).
//
// The table: `cap` 32-bit slots, DICT_EMPTY or a row number.  A slot that was
// claimed belongs to one class of equal values for good: it only ever changes
// from one row of the class to a smaller row of the same class (fetch_min).
// Nothing is ever removed, so every row of a class walks the same probe
// sequence past the same foreign slots and ends in the class's one slot; when
// all inserts are done that slot holds the class's smallest row, whatever the
// order the lanes ran in.  No loop waits for another lane: a lane that loses
// the claim compares against the winner's row (whose bytes an earlier launch
// wrote) and goes on.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LP_DICT_HD __host__ __device__ __forceinline__
#else
#define LP_DICT_HD inline
#endif

namespace lp {

constexpr uint32_t DICT_EMPTY = 0xFFFFFFFFu;

// slots for `count` rows: load factor <= 0.5 (every row distinct), never 0
LP_DICT_HD uint32_t dict_capacity(int64_t count) { return (uint32_t)(2 * (uint64_t)(count > 0 ? count : 0) + 1); }

LP_DICT_HD uint64_t dict_mix(uint64_t h, uint64_t w) {
    h ^= w;
    h *= 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 32);
}

// 64-bit hash of a value of n bytes given as its little-endian 8-byte words
// (word(j) = bytes [8j, 8j + 8), the last one zero-padded), the length mixed
// in first: the same for every representation of the same bytes
template <class Word>
LP_DICT_HD uint64_t dict_hash(uint32_t n, Word word) {
    uint64_t h = dict_mix(0x243F6A8885A308D3ull, n);
    for (uint32_t j = 0; 8 * j < n; ++j) h = dict_mix(h, word(j));
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}

// the home slot; bits 1..32 (LP_OPT_DICT_HASH_BITS, tests): only that many low
// bits of the hash count, so that distinct values collide
LP_DICT_HD uint32_t dict_home(uint64_t h, uint32_t cap, int bits) {
    if (bits > 0) return (uint32_t)((bits >= 64 ? h : h & ((1ull << bits) - 1)) % cap);
    return (uint32_t)(((h >> 32) * (uint64_t)cap) >> 32);
}

// Row k (valid, not yet in the table) with home slot `home`: the slot of its
// class, claimed when no row of the class came before.  same(r): row r's
// value equals row k's (lengths, then bytes).  The probe is bounded by the
// capacity: DICT_EMPTY when it ran out (a table without a free slot: never
// with dict_capacity).  When the slot already holds a smaller row of the
// class -- the common case of a hot key with rows taken in ascending order --
// no atomic is issued at all.
template <class At, class Slots, class Same>
LP_DICT_HD uint32_t dict_insert(Slots slots, uint32_t cap, uint32_t home, uint32_t k, Same same) {
    uint32_t s = home;
    for (uint32_t probe = 0; probe < cap; ++probe) {
        uint32_t cur = At::load(slots + s);
        if (cur == DICT_EMPTY) {
            cur = At::cas(slots + s, DICT_EMPTY, k);
            if (cur == DICT_EMPTY) return s;  // claimed
        }
        if (cur == k || same(cur)) {
            if (cur > k) At::fetch_min(slots + s, k);
            return s;
        }
        s = s + 1 == cap ? 0 : s + 1;
    }
    return DICT_EMPTY;
}

#if defined(__HIPCC__)
// agent scope: the XCDs do not share an L2, a slot is read through the
// atomic's return value or an agent-scope atomic load
struct DictAtDevice {
    template <class P>
    static __device__ __forceinline__ uint32_t load(P p) {
        return __hip_atomic_load((const uint32_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    template <class P>
    static __device__ __forceinline__ uint32_t cas(P p, uint32_t expect, uint32_t v) {
        __hip_atomic_compare_exchange_strong((uint32_t*)p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        return expect;  // the old value
    }
    template <class P>
    static __device__ __forceinline__ void fetch_min(P p, uint32_t v) {
        __hip_atomic_fetch_min((uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
#endif

#if !defined(__HIP_DEVICE_COMPILE__)
struct DictAtHost {
    static inline uint32_t load(const uint32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static inline uint32_t cas(uint32_t* p, uint32_t expect, uint32_t v) {
        __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expect;
    }
    static inline void fetch_min(uint32_t* p, uint32_t v) {
        uint32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (cur > v && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
};
#endif

}  // namespace lp
