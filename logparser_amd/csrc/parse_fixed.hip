// The fixed-shape instances of the chunked parse kernel (lp_fixed.h): one
// k_parse_chunks instance per shape, built on the SIMPLE one, with the
// shape's elements and stage lists folded in (lp_device.h phase1<...,
// SHAPE>).  A translation unit of its own so that make -j compiles it beside
// parse.hip.  The deferred pass and the queued lines run the generic kernels
// of parse.hip: they do no work in a normal launch, and their results are
// the same by construction.
#include "parse_chunk.h"

namespace lp {

namespace {
template <int SHAPE>
void run_fixed(const ParseLaunch& a, const DeviceArgs* d_args, const ChunkPlan& cp, unsigned grid, hipStream_t s) {
    hipLaunchKernelGGL((k_parse_chunks<false, true, false, SHAPE>), dim3(grid), dim3(PW), cp.lds, s, a.buf, a.nbytes,
                       d_args, cp.cb, cp.win_cap, a.force_direct ? 1 : 0, a.chunk_wait);
}
}  // namespace

int launch_chunks_fixed(const ParseLaunch& a, const DeviceArgs* d_args, const ChunkPlan& cp, unsigned grid,
                        hipStream_t s) {
    switch (a.shape) {
    case FS_COMBINED: run_fixed<FS_COMBINED>(a, d_args, cp, grid, s); return 0;
    case FS_COMMON: run_fixed<FS_COMMON>(a, d_args, cp, grid, s); return 0;
    }
    return -1;  // no instance of that shape: an error, never another kernel
}

#if defined(LP_PROFILE)
int prof_read_parse_fixed(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * PROF_WAVES * PROF_POINTS) == hipSuccess ? 0 : -1;
}
int prof_clear_parse_fixed() {
    static unsigned long long z[PROF_WAVES * PROF_POINTS];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

}  // namespace lp
