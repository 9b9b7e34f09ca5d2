// gfx950 kernels of lp_result_select on a device view (include/logparser_amd.h):
// the lines of a window whose status is in a mask, ascending -- the rows a
// record reader keeps (ApacheHttpdLogfileRecordReader.java:246-277 skips a line
// that throws DissectionFailure; ApacheHttpdlogDeserializer.java:284-291 returns
// null for it) or the ones the host must redo (FALLBACK) -- as an ordered
// stream compaction of the status column:
//
//   k_select_count  one lane per 16 lines: the lane's match word, the block's
//                   match count
//   (scan)          the block counts -> block bases (hipCUB exclusive sum; its
//                   last item is the total, which the host reads)
//   k_select_write  the match words again, each lane's rank from a wave prefix
//                   of the popcounts and the waves' totals in LDS, its matches
//                   stored as consecutive int64 line indices
//
// lp_result_select_where runs the same two passes over the bits k_where_eval
// (where.hip) left: the kernels' BITS instances take a group's match word from
// them (one 16-bit load) instead of from the status bytes.  The status
// instances are the code they were.
//
// No atomics: the output order is the line order.  The window is cut into
// 16-line groups aligned in the status column (its base is 256-byte aligned):
// a group wholly inside the window is one aligned 16-byte load, the window's
// first and last group are read byte by byte.
#include <hip/hip_runtime.h>

#define LP_KERNEL_TU 1  // device column pointers are global-memory pointers (lp_program.h)

#include <hipcub/hipcub.hpp>

#include "kernels_common.h"

namespace lp {

namespace {

constexpr int SEL_GROUP = 16;                         // lines per lane
constexpr int SEL_TB = SEL_BLOCK_LINES / SEL_GROUP;   // threads per block
constexpr int SEL_WV = SEL_TB / 64;                   // waves per block
static_assert(SEL_WAVE_LINES == 64 * SEL_GROUP && SEL_BLOCK_LINES % SEL_WAVE_LINES == 0, "select tiles");

// The match word of the 16 lines [g, g + 16) (g a multiple of 16): bit b set
// when line g + b is inside [lo, hi) and its status is in mask.
__device__ __forceinline__ uint32_t sel_match(const LP_G uint8_t* status, int64_t g, int64_t lo, int64_t hi, uint32_t mask) {
    uint32_t m = 0;
    if (g >= lo && g + SEL_GROUP <= hi) {
        const u32x4 v = *reinterpret_cast<const LP_G u32x4*>(status + g);
#pragma unroll
        for (int b = 0; b < SEL_GROUP; ++b) m |= ((mask >> ((v[b >> 2] >> (8 * (b & 3))) & 7u)) & 1u) << b;
    } else {
        for (int b = 0; b < SEL_GROUP; ++b) {
            const int64_t i = g + b;
            if (i >= lo && i < hi) m |= ((mask >> (status[i] & 7u)) & 1u) << b;
        }
    }
    return m;
}

// The same from k_where_eval's bits (lp_table.h WhereArgs::bits: bit j is line
// (first & ~15) + j, so a group is one aligned 16-bit word); a group past the
// window's end has no word.
__device__ __forceinline__ uint32_t sel_match_bits(const LP_G uint16_t* bits, int64_t g, int64_t lo, int64_t hi) {
    return g < hi ? (uint32_t)bits[(g - (lo & ~(int64_t)(SEL_GROUP - 1))) / SEL_GROUP] : 0u;
}

// the match word's source: the status column (src: its bytes) or the bits (src: their words)
template <bool BITS>
__device__ __forceinline__ uint32_t sel_word(const uint8_t* src, int64_t g, int64_t lo, int64_t hi, uint32_t mask) {
    if constexpr (BITS) return sel_match_bits((const LP_G uint16_t*)src, g, lo, hi);
    else return sel_match((const LP_G uint8_t*)src, g, lo, hi, mask);
}

// this lane's group of block blk: the groups start at the window's first line rounded down to 16
__device__ __forceinline__ int64_t sel_group(int64_t first, int64_t blk, int wv, int lane) {
    return (first & ~(int64_t)(SEL_GROUP - 1)) + blk * SEL_BLOCK_LINES + (int64_t)wv * SEL_WAVE_LINES + (int64_t)lane * SEL_GROUP;
}

template <bool BITS>
__global__ __launch_bounds__(SEL_TB) void k_select_count(const uint8_t* status, int64_t first, int64_t count, uint32_t mask,
                                                         int64_t* block_cnt, int64_t n_blocks) {
    __shared__ uint32_t s_wave[SEL_WV];
    const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
    const int64_t g = sel_group(first, (int64_t)blockIdx.x, wv, lane);
    const uint32_t m = sel_word<BITS>(status, g, first, first + count, mask);
    const uint32_t w = wave_sum((uint32_t)__popc(m));
    if (lane == 0) s_wave[wv] = w;
    __syncthreads();
    if (wv == 0 && lane == 0) {
        uint32_t t = 0;
        for (int q = 0; q < SEL_WV; ++q) t += s_wave[q];
        block_cnt[blockIdx.x] = (int64_t)t;
        if (blockIdx.x == 0) block_cnt[n_blocks] = 0;  // the scan's last item: the total
    }
}

template <bool BITS>
__global__ __launch_bounds__(SEL_TB) void k_select_write(const uint8_t* status, int64_t first, int64_t count, uint32_t mask,
                                                         const int64_t* block_base, int64_t* rows) {
    __shared__ uint32_t s_wave[SEL_WV];
    const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
    const int64_t g = sel_group(first, (int64_t)blockIdx.x, wv, lane);
    uint32_t m = sel_word<BITS>(status, g, first, first + count, mask);
    const uint32_t c = (uint32_t)__popc(m);
    const uint32_t incl = wave_incl_scan(c);
    if (lane == 63) s_wave[wv] = incl;
    __syncthreads();
    uint32_t before = incl - c;  // matches of the block's earlier lanes
    for (int q = 0; q < wv; ++q) before += s_wave[q];
    // (the host checked the total against rows_cap: every position is inside the buffer)
    LP_G int64_t* out = (LP_G int64_t*)rows + (block_base[blockIdx.x] + (int64_t)before);
    while (m) {
        *out++ = g + (int64_t)__builtin_ctz(m);
        m &= m - 1u;
    }
}

struct SelLayout {
    size_t tmp, tmp_bytes, cnt, base, bits, total;
    int64_t n_blocks;
};
SelLayout sel_layout(int64_t first, int64_t count) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    SelLayout L{};
    const int64_t span = (first & (SEL_GROUP - 1)) + count;
    L.n_blocks = (span + SEL_BLOCK_LINES - 1) / SEL_BLOCK_LINES;
    const size_t items = (size_t)L.n_blocks + 1;
    hipcub::DeviceScan::ExclusiveSum(nullptr, L.tmp_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int)items);
    L.tmp = 0;
    L.cnt = al(L.tmp_bytes);
    L.base = L.cnt + al(8 * items);
    L.bits = L.base + al(8 * items);  // k_where_eval's words: one per 64 lines of the span
    L.total = L.bits + al(8 * (size_t)((span + 63) / 64));
    return L;
}

}  // namespace

size_t select_scratch_bytes(int64_t first, int64_t count) { return sel_layout(first, count).total; }

uint64_t* select_bits(int64_t first, int64_t count, void* scratch, size_t scratch_bytes) {
    if (first < 0 || count <= 0) return nullptr;
    const SelLayout L = sel_layout(first, count);
    return L.total > scratch_bytes ? nullptr : reinterpret_cast<uint64_t*>((char*)scratch + L.bits);
}

int launch_select_count(const uint8_t* status, int64_t first, int64_t count, uint32_t mask, void* scratch,
                        size_t scratch_bytes, hipStream_t s, const int64_t** total, bool from_bits) {
    if (first < 0 || count <= 0) return -1;
    const SelLayout L = sel_layout(first, count);
    if (L.total > scratch_bytes || L.n_blocks >= 0x7FFFFFFF) return -1;
    int64_t* cnt = reinterpret_cast<int64_t*>((char*)scratch + L.cnt);
    int64_t* base = reinterpret_cast<int64_t*>((char*)scratch + L.base);
    if (from_bits)
        hipLaunchKernelGGL(k_select_count<true>, dim3((unsigned)L.n_blocks), dim3(SEL_TB), 0, s,
                           (const uint8_t*)scratch + L.bits, first, count, mask, cnt, L.n_blocks);
    else
        hipLaunchKernelGGL(k_select_count<false>, dim3((unsigned)L.n_blocks), dim3(SEL_TB), 0, s, status, first, count, mask,
                           cnt, L.n_blocks);
    size_t t = L.tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum((char*)scratch + L.tmp, t, (const int64_t*)cnt, base, (int)L.n_blocks + 1, s) !=
        hipSuccess)
        return -1;
    *total = base + L.n_blocks;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_select_write(const uint8_t* status, int64_t first, int64_t count, uint32_t mask, int64_t* rows, void* scratch,
                        size_t scratch_bytes, hipStream_t s, bool from_bits) {
    if (first < 0 || count <= 0 || !rows) return -1;
    const SelLayout L = sel_layout(first, count);
    if (L.total > scratch_bytes) return -1;
    const int64_t* base = reinterpret_cast<const int64_t*>((char*)scratch + L.base);
    if (from_bits)
        hipLaunchKernelGGL(k_select_write<true>, dim3((unsigned)L.n_blocks), dim3(SEL_TB), 0, s,
                           (const uint8_t*)scratch + L.bits, first, count, mask, base, rows);
    else
        hipLaunchKernelGGL(k_select_write<false>, dim3((unsigned)L.n_blocks), dim3(SEL_TB), 0, s, status, first, count, mask,
                           base, rows);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lp
