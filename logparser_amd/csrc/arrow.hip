// gfx950 kernels of the Arrow C Data Interface export on device memory
// (include/logparser_amd.h lp_result_arrow / lp_arrow_from_tables): what Arrow
// wants and the table kernels do not write.
//
//   k_arrow_validity  the columns' valid bytes -> Arrow validity bitmaps (bit
//                     k & 7 of byte k >> 3) and the count of valid rows, every
//                     column of the call in one launch (column on blockIdx.y)
//   k_arrow_narrow32  a map column's int64 entry offsets -> Arrow's int32
//
// The validity tiles are select.hip's: one lane takes 16 rows with one aligned
// 16-byte load and makes a 16-bit word, a wave covers ARROW_WAVE_ROWS rows and
// stores one contiguous 128-byte piece of bitmap, a block ARROW_BLOCK_ROWS.
// The 16-row groups are aligned in MEMORY; a lane's output word is aligned in
// the BITMAP.  When valid is 16-byte aligned (every table this library
// allocates) the two agree.  When it is not (lp_arrow_from_tables takes any
// pointer), s = valid & 15: the lane loads the aligned group that starts s
// bytes before its rows and takes the missing s rows from the next lane's
// group (one shuffle; the wave's last lane loads that group itself).  A group
// not wholly inside [0, n) -- the head in front of the first aligned group, the
// tail -- is read byte by byte and its missing rows are 0; the same kernel
// writes the zeros from n up to the end of the 64-byte multiple.
//
// Stores: 2 bytes per lane, 128 contiguous bytes per wave instruction (the ISA
// shows one global_store_short per lane and no read-modify-write; a wave's
// piece is a whole 128-byte line of the bitmap, which is 256-byte aligned, so
// no line is written by two waves).  Wider stores would need a cross-lane
// gather of the words for a kernel that moves 1/8 byte per row it reads; kept
// simple.
#include <hip/hip_runtime.h>

#define LP_KERNEL_TU 1  // device column pointers are global-memory pointers (lp_program.h)

#include "kernels_common.h"

namespace lp {

namespace {

constexpr int AV_GROUP = 16;                           // rows per lane
constexpr int AV_TB = ARROW_BLOCK_ROWS / AV_GROUP;     // threads per block
constexpr int AV_WV = AV_TB / 64;                      // waves per block
static_assert(ARROW_WAVE_ROWS == 64 * AV_GROUP && ARROW_BLOCK_ROWS % ARROW_WAVE_ROWS == 0, "validity tiles");

// the high bit of every non-zero byte of w
__device__ __forceinline__ uint32_t nz_hb(uint32_t w) { return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u; }

// The word of the 16 rows [q, q + 16) (valid + q 16-byte aligned; q may be
// negative): bit b set when row q + b is inside [0, n) and valid[q + b] != 0.
__device__ __forceinline__ uint32_t av_word(const LP_G uint8_t* valid, int64_t n, int64_t q) {
    uint32_t m = 0;
    if (q >= 0 && q + AV_GROUP <= n) {
        const u32x4 v = *reinterpret_cast<const LP_G u32x4*>(valid + q);
        m = bits16(nz_hb(v[0]), nz_hb(v[1]), nz_hb(v[2]), nz_hb(v[3]));
    } else {
        for (int b = 0; b < AV_GROUP; ++b) {
            const int64_t i = q + b;
            if (i >= 0 && i < n) m |= (valid[i] != 0 ? 1u : 0u) << b;
        }
    }
    return m;
}

__global__ __launch_bounds__(AV_TB) void k_arrow_validity(const ArrowValidArgs A, int64_t n, int64_t bits) {
    __shared__ uint32_t s_wave[AV_WV];
    const LP_G uint8_t* valid = (const LP_G uint8_t*)A.col[blockIdx.y].valid;
    const int lane = lane_id(), wv = (int)(threadIdx.x >> 6);
    // this lane's rows [g, g + 16): bitmap bytes g / 8 and g / 8 + 1
    const int64_t g = (int64_t)blockIdx.x * ARROW_BLOCK_ROWS + (int64_t)wv * ARROW_WAVE_ROWS + (int64_t)lane * AV_GROUP;
    const uint32_t s = (uint32_t)((uintptr_t)valid & 15u);  // (the same in every lane of the column's blocks)
    uint32_t w = av_word(valid, n, g - (int64_t)s);
    if (s) {
        uint32_t next = (uint32_t)__shfl_down((int)w, 1);
        if (lane == 63) next = av_word(valid, n, g - (int64_t)s + AV_GROUP);
        w = ((w >> s) | (next << (16u - s))) & 0xFFFFu;
    }
    // (bits is a multiple of 512: a lane's two bytes are inside the bitmap or wholly past it)
    if (g < bits) *reinterpret_cast<LP_G uint16_t*>((LP_G uint8_t*)A.col[blockIdx.y].bitmap + (g >> 3)) = (uint16_t)w;
    const uint32_t c = wave_sum((uint32_t)__popc(w));
    if (lane == 0) s_wave[wv] = c;
    __syncthreads();
    if (wv == 0 && lane == 0) {
        uint32_t t = 0;
        for (int q = 0; q < AV_WV; ++q) t += s_wave[q];
        if (t) atomicAdd(A.col[blockIdx.y].count, (unsigned long long)t);
    }
}

constexpr int NW_TB = 256;  // threads per block, 4 offsets each

// out[k] = (int32) in[k], k < n.  vec: both arrays are 16-byte aligned, then a
// lane's four values are two 16-byte loads and one 16-byte store.  The range
// is the host's to check (the last offset is the entry count it knows).
__global__ __launch_bounds__(NW_TB) void k_arrow_narrow32(const int64_t* in, int32_t* out, int64_t n, int vec) {
    const int64_t k = 4 * ((int64_t)blockIdx.x * NW_TB + (int64_t)threadIdx.x);
    if (vec && k + 4 <= n) {
        const u32x4 a = *reinterpret_cast<const LP_G u32x4*>((const LP_G int64_t*)in + k);
        const u32x4 b = *reinterpret_cast<const LP_G u32x4*>((const LP_G int64_t*)in + k + 2);
        *reinterpret_cast<LP_G u32x4*>((LP_G int32_t*)out + k) = u32x4{a[0], a[2], b[0], b[2]};
    } else {
        for (int j = 0; j < 4 && k + j < n; ++j) out[k + j] = (int32_t)in[k + j];
    }
}

}  // namespace

int launch_arrow_validity(const ArrowValidArgs& A, int n_cols, int64_t n_rows, hipStream_t s) {
    if (n_cols <= 0 || n_cols > ARROW_MAX_COLS || n_rows <= 0) return -1;
    const int64_t bits = 8 * (((((int64_t)n_rows + 7) >> 3) + 63) & ~(int64_t)63);
    const int64_t blocks = (bits + ARROW_BLOCK_ROWS - 1) / ARROW_BLOCK_ROWS;
    if (blocks >= 0x7FFFFFFF) return -1;
    hipLaunchKernelGGL(k_arrow_validity, dim3((unsigned)blocks, (unsigned)n_cols), dim3(AV_TB), 0, s, A, n_rows, bits);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_arrow_narrow32(const int64_t* in, int32_t* out, int64_t n, hipStream_t s) {
    if (n <= 0 || !in || !out) return -1;
    const int64_t blocks = (n + 4 * NW_TB - 1) / (4 * NW_TB);
    if (blocks >= 0x7FFFFFFF) return -1;
    const int vec = (((uintptr_t)in | (uintptr_t)out) & 15u) == 0 ? 1 : 0;
    hipLaunchKernelGGL(k_arrow_narrow32, dim3((unsigned)blocks), dim3(NW_TB), 0, s, in, out, n, vec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lp
