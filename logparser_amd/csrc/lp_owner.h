// Owner lookup of the wave-cooperative passes (uri.hip: the block gather,
// the event walk, the query piece pass) as mask arithmetic.  Each lane holds
// a line with cnt items; the items of all lines are numbered line after line
// (first[l] = the sum of the counts of the lanes before l), and the wave
// works them off in rounds of 64, lane i of a round taking item g = g0 + i.
//
// Definition: the owner of item g is THE LAST LANE WHOSE FIRST ITEM IS <= g.
// For g below the wave's total that is the non-empty lane whose items
// include g: an empty lane shares its first item with the next non-empty
// lane, which lies after it (and the empty lanes behind the last non-empty
// one start at the total, above g).  Items at or past the total have no
// owner; for them the functions here return the last non-empty lane.
//
// No search is needed: the owner is the rank-th non-empty lane, rank = the
// number of non-empty lanes whose first item is <= g, and that is
//   K = the non-empty lanes whose first item is <  g0   (wave-uniform), plus
//       the non-empty lanes whose first item is in [g0, g0 + i]: the bits of
//   H = the round's head mask (bit j: a non-empty lane's first item is g0 + j)
//       at or below i.
// With N = the mask of non-empty lanes: owner = select64(N, rank - 1).
//
// Only integer arithmetic on the masks, no cross-lane operation: host and
// device compile the same code (tests/emu/owner_emu.cpp checks it against
// the definition on the CPU).
#pragma once
#include <stdint.h>

#if !defined(__HIP__)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace lp {

// k-th set bit (0-based) of m (k < popcount(m))
__host__ __device__ inline uint32_t select64(uint64_t m, uint32_t k) {
    uint32_t pos = 0, v = (uint32_t)m, c = (uint32_t)__builtin_popcount(v);
    if (k >= c) { k -= c; v = (uint32_t)(m >> 32); pos = 32; }
    c = (uint32_t)__builtin_popcount(v & 0xFFFFu);
    if (k >= c) { k -= c; v >>= 16; pos += 16; }
    c = (uint32_t)__builtin_popcount(v & 0xFFu);
    if (k >= c) { k -= c; v >>= 8; pos += 8; }
    c = (uint32_t)__builtin_popcount(v & 0xFu);
    if (k >= c) { k -= c; v >>= 4; pos += 4; }
    c = (uint32_t)__builtin_popcount(v & 3u);
    if (k >= c) { k -= c; v >>= 2; pos += 2; }
    return pos + (k >= (v & 1u) ? 1u : 0u);
}

// the round's heads at or below slot i (0..63)
__host__ __device__ inline uint64_t owner_heads_upto(uint64_t H, int i) { return H & ((2ull << i) - 1ull); }

// The rank of slot i's owner among the non-empty lanes, counted from 1: the
// number of non-empty lanes whose first item is <= g0 + i.
__host__ __device__ inline uint32_t owner_rank(uint32_t K, uint64_t H, int i) {
    return K + (uint32_t)__builtin_popcountll(owner_heads_upto(H, i));
}

// The owner lane of slot i of a round (N, K, H as above).  0 for a wave
// without items (N == 0), which has no round.  (uri.hip reads
// select64(N, r) and that lane's first item from a table in LDS that every
// non-empty lane fills at its own rank, popcount(N below the lane).)
__host__ __device__ inline int owner_lane(uint64_t N, uint32_t K, uint64_t H, int i) {
    const uint32_t rank = owner_rank(K, H, i);
    return rank ? (int)(select64(N, rank - 1) & 63u) : 0;
}

}  // namespace lp
