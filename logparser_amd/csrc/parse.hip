// gfx950 parse kernels of the logparser_amd engine (phase 1: LogFormat match,
// token flags, time stamps, first line; lp_device.h phase1).
//
//   k_parse_chunks     the line index and phase 1 in ONE pass over the input.  One
//                      wave per byte chunk: the chunk's window (with the tail of
//                      its last line) staged in LDS with its class masks and line
//                      terminators, the lines starting in the chunk numbered by a
//                      decoupled look-back over the chunks' line counts, one lane
//                      per line (the kernel itself: parse_chunk.h, shared with the
//                      fixed-shape instances of parse_fixed.hip).  Several
//                      LogFormats: also every line's match word
//   k_parse_deferred   the chunks whose wave gave up waiting for its line number
//                      (none in a normal launch)
//   k_route_ovf        several LogFormats: the match words of the queued lines,
//                      before the routing scan (kernels.hip)
//   k_parse_ovf_lines  the lines a chunk queued (more than 64 lines, a line ending
//                      past its window, a line that needs the backtracking DFS or
//                      the routing scan): read from HBM directly
#include "parse_chunk.h"

namespace lp {

namespace {

// The lines k_parse_chunks queued, 64 per wave on a persistent grid, read
// from HBM.  Without URI stages (whose kernel re-counts every line) their
// status counts go to the batch counters here.
__global__ __launch_bounds__(PW) void k_parse_ovf_lines(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                        const DeviceArgs* __restrict__ args, uint32_t stk_words) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    if (C.meta->cap_ovf) return;
    const uint64_t nq = min((uint64_t)C.meta->ovf_lines, (uint64_t)C.cap_lines + 1);  // (queue_line checked the rest)
    const uint64_t n_lines = C.meta->n_lines;
    if ((uint64_t)blockIdx.x * PW >= nq) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Elem* s_elems = reinterpret_cast<Elem*>(smem);
    WaveStack stk{reinterpret_cast<uint32_t*>(smem + 16 * P.n_elems) + lane_id()};
    load_elems(P, s_elems);
    __syncthreads();
    WaveCounts WC;
    for (uint64_t q0 = (uint64_t)blockIdx.x * PW; q0 < nq; q0 += (uint64_t)gridDim.x * PW) {
        const uint64_t q = q0 + lane_id();
        bool active = q < nq;
        const int64_t li = active ? (int64_t)C.ovf_lines[q] : 0;
        uint64_t s = 0, e = 0;
        if (active) {
            // a queued line is one of the batch's lines, and its index entries
            // bound a line of the buffer (the sentinel is nbytes or nbytes + 1)
            uint64_t e1 = 0;
            const bool in = (uint64_t)li < n_lines;
            if (in) {
                s = C.line_off[li];
                e1 = C.line_off[li + 1];
            }
            if (!in || s >= e1 || e1 > nbytes + 1) {
                check_fail(C, CHK_OVF_LINE, q, (uint64_t)li, s, e1);
                active = false;
                s = 0;
            } else {
                e = e1 - 1;
            }
        }
        const uint64_t len = e - s;
        const int n0 = (int)(len > (uint64_t)0x7FFFFFFF ? 0x7FFFFFFF : len);
        const int n = active ? crlf_len(n0, n0 > 0 ? buf[e - 1] : 0u) : 0;
        const LP_G uint8_t* ls = (const LP_G uint8_t*)(buf) + s;
        const uint32_t mis = (uint32_t)((uintptr_t)ls & 3);
        const LineT<const LP_G uint8_t*> L{ls - mis, mis, n};
        parse_wave(P, s_elems, C, L, active, li, stk, false, WC);
    }
    if (!P.has_phase2() && lane_id() == 0 && WC.act) {
        atomicAdd(&C.meta->counters[0], (unsigned long long)WC.act);
        atomicAdd(&C.meta->counters[1], (unsigned long long)WC.ok);
        atomicAdd(&C.meta->counters[2], (unsigned long long)WC.bad);
        atomicAdd(&C.meta->counters[3], (unsigned long long)(WC.act - WC.ok - WC.bad));
    }
}

// Several LogFormats, one pass: the match words (with the DFS) of the lines
// the chunk kernel queued, 64 per wave on a persistent grid, from HBM; the
// routing scan (k_fmt_*) runs after it.
__global__ __launch_bounds__(PW) void k_route_ovf(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                  const DeviceArgs* __restrict__ args, uint32_t stk_words) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    if (C.meta->cap_ovf) return;
    const uint64_t nq = min((uint64_t)C.meta->ovf_lines, (uint64_t)C.cap_lines + 1);
    const uint64_t n_lines = C.meta->n_lines;
    if ((uint64_t)blockIdx.x * PW >= nq) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Elem* s_elems = reinterpret_cast<Elem*>(smem);
    WaveStack stk{reinterpret_cast<uint32_t*>(smem + 16 * P.n_elems) + lane_id()};
    load_elems(P, s_elems);
    __syncthreads();
    for (uint64_t q0 = (uint64_t)blockIdx.x * PW; q0 < nq; q0 += (uint64_t)gridDim.x * PW) {
        const uint64_t q = q0 + lane_id();
        if (q >= nq) continue;
        const int64_t li = (int64_t)C.ovf_lines[q];
        if ((uint64_t)li >= n_lines) continue;  // (k_parse_ovf_lines reports it)
        const uint64_t s = C.line_off[li], e1 = C.line_off[li + 1];
        if (s >= e1 || e1 > nbytes + 1) continue;  // (idem)
        const uint64_t e = e1 - 1, len = e - s;
        const int n0 = (int)(len > (uint64_t)0x7FFFFFFF ? 0x7FFFFFFF : len);
        const int n = crlf_len(n0, n0 > 0 ? buf[e - 1] : 0u);
        const LP_G uint8_t* ls = (const LP_G uint8_t*)(buf) + s;
        const uint32_t mis = (uint32_t)((uintptr_t)ls & 3);
        const LineT<const LP_G uint8_t*> L{ls - mis, mis, n};
        C.fmt_match[li] = (uint16_t)fmt_match_word(P, s_elems, L, stk, false);
    }
}

}  // namespace

// The chunked kernel's LDS: a window of the most waves per CU that still
// holds the chunk (target_lines x the mean line) plus 64 bytes before it and
// an overhang of at least 2 mean lines for the tail of its last line.
ChunkPlan chunk_plan(const ParseLaunch& a) {
    ChunkPlan c{};
    c.stk_words = (uint32_t)(a.stack_depth > 0 ? a.stack_depth : 1) * PW;
    // the chunk kernels run no DFS (ST_REDO lines are queued): no stack in
    // their LDS (the queued lines' kernels have theirs, stk_words)
    const uint64_t fixed = 16 * (uint64_t)a.n_elems + 16 * ((4 * MAXS + 15) / 16);
    const uint64_t per8 = 8 + MC_N;  // LDS bytes per 8 window bytes (window + mask planes)
    const uint64_t mean = a.mean_line ? a.mean_line : 256;
    const uint64_t oh = std::max<uint64_t>(512, ((2 * mean + 63) & ~63ull));
    // lines per chunk: at most 54 (measured best at 8 waves per CU, config 2:
    // tools/chunk_sweep.py), and the count that puts the most lines in
    // flight per CU (waves x lines) over the wave counts the registers allow
    // (the several-format instance: LP_MF_WPE waves per SIMD); LP_OPT_CHUNK_LINES
    // fixes the count
    uint64_t lines = a.chunk_lines ? a.chunk_lines : 54;
    if (!a.chunk_lines) {
        const int maxw = a.multi ? 4 * LP_MF_WPE : LP_CHUNK_MAXW;
        const uint64_t lmax = a.multi ? LP_CHUNK_LMAX_MF : LP_CHUNK_LMAX;
        uint64_t best = 0;
        for (int k = 8; k <= maxw; ++k) {
            const uint64_t budget = 160 * 1024 / k - 640;
            if (budget <= fixed) break;
            const uint64_t capk = std::min<uint64_t>(((budget - fixed) * 8 / per8) & ~63ull, 48 * 1024) & ~1023ull;
            const uint64_t lk = capk > 64 + oh + 63 ? std::min<uint64_t>(lmax, (capk - 64 - oh - 63) / mean) : 0;
            if (lk >= 16 && (uint64_t)k * lk > best) {
                best = (uint64_t)k * lk;
                lines = lk;
            }
        }
    }
    uint64_t cb = ((lines * mean) + 63) & ~63ull;
    if (cb < 1024) cb = 1024;
    const uint64_t need = cb + 64 + oh;
    uint64_t cap = 0;
    int waves = 0;
    for (int k = LP_CHUNK_MAXW; k >= 2 && !cap; --k) {
        const uint64_t budget = 160 * 1024 / k - 640;
        if (budget <= fixed) continue;
        const uint64_t w = ((budget - fixed) * 8 / per8) & ~63ull;
        if (w >= need || k == 2) {
            // whole 1 KiB LDS-DMA blocks, no more than the chunk needs (a
            // wave stages its whole window: a larger one only re-reads the
            // next chunk's bytes)
            cap = std::min<uint64_t>(std::min<uint64_t>(w, 48 * 1024), (need + 1023) & ~1023ull) & ~1023ull;
            waves = k;
        }
    }
    if (cap < need) cb = cap > 64 + oh + 1024 ? ((cap - 64 - oh) & ~63ull) : 1024;  // long lines: fewer per chunk
    if (cap < cb + 64 + 64) cap = (cb + 128 + 1023) & ~1023ull;
    c.cb = (uint32_t)cb;
    c.win_cap = (uint32_t)cap;
    c.waves_per_cu = waves;
    c.lds = fixed + cap + MC_N * (cap / 8);
    c.n_chunks = a.nbytes ? (int64_t)((a.nbytes + cb - 1) / cb) : 0;
    return c;
}

#if defined(LP_PROFILE)
// (the points of this unit's kernels plus the fixed-shape instances': one of
// the two chunk kernels ran since the last clear, the other's are zero)
int prof_read_parse(unsigned long long* out) {
    static unsigned long long f[PROF_WAVES * PROF_POINTS];
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof f) != hipSuccess || prof_read_parse_fixed(f) != 0) return -1;
    for (int i = 0; i < PROF_WAVES * PROF_POINTS; ++i) out[i] += f[i];
    return 0;
}
int prof_clear_parse() {
    static unsigned long long z[PROF_WAVES * PROF_POINTS];
    return hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof z) == hipSuccess && prof_clear_parse_fixed() == 0 ? 0 : -1;
}
#endif


int launch_parse(const ParseLaunch& a, const DeviceArgs* d_args, const Columns& C, hipStream_t s) {
    const int64_t waves = parse_waves(a.cap_lines);
    const int64_t grid = std::max<int64_t>(1, waves < 1024 ? waves : 1024);
    // one pass: line index + phase 1, then the queued lines from HBM
    const ChunkPlan cp = chunk_plan(a);
    if (cp.n_chunks > 0) {
        // the instance per program shape: literal-aware first candidates
        // only for programs that have such an element, SIMPLE for the
        // Apache common / combined family; the chunks, then the deferred pass (its blocks return at once
        // when no wave gave up waiting, the normal case)
        const unsigned g0 = (unsigned)cp.n_chunks + 1, g1 = (unsigned)std::min<int64_t>(cp.n_chunks, 1024);
        const int fd = a.force_direct ? 1 : 0;
        // (the instance per program shape: LA, SIMPLE)
        auto run = [&](auto chunks, auto deferred) {
            hipLaunchKernelGGL(chunks, dim3(g0), dim3(PW), cp.lds, s, a.buf, a.nbytes, d_args, cp.cb, cp.win_cap, fd,
                               a.chunk_wait);
            hipLaunchKernelGGL(deferred, dim3(g1), dim3(PW), cp.lds, s, a.buf, a.nbytes, d_args, cp.cb, cp.win_cap, fd);
        };
        const bool simple = a.simple;
        // (several LogFormats: one instance; their first leaves are walked per lane)
        // (a fixed shape: its own chunk instance, the SIMPLE deferred pass)
        if (a.shape != FS_NONE && !a.multi && !a.lit_aware && simple) {
            if (launch_chunks_fixed(a, d_args, cp, g0, s) != 0) return -1;
            hipLaunchKernelGGL((k_parse_deferred<false, true, false>), dim3(g1), dim3(PW), cp.lds, s, a.buf, a.nbytes,
                               d_args, cp.cb, cp.win_cap, fd);
        } else if (a.multi) run(k_parse_chunks<true, false, true>, k_parse_deferred<true, false, true>);
        else if (a.lit_aware && simple) run(k_parse_chunks<true, true, false>, k_parse_deferred<true, true, false>);
        else if (a.lit_aware) run(k_parse_chunks<true, false, false>, k_parse_deferred<true, false, false>);
        else if (simple) run(k_parse_chunks<false, true, false>, k_parse_deferred<false, true, false>);
        else run(k_parse_chunks<false, false, false>, k_parse_deferred<false, false, false>);
        // (LDS of the queued lines' kernels: the elements and the DFS stack)
        const size_t lds_ovf = 16 * (size_t)a.n_elems + 4 * (size_t)cp.stk_words;
        if (a.multi) {
            // the queued lines' match words, then the sticky routing scan
            // over every line's word (fmt_id of every line, the state after
            // the batch)
            hipLaunchKernelGGL(k_route_ovf, dim3((unsigned)grid), dim3(PW), lds_ovf, s, a.buf, a.nbytes, d_args,
                               cp.stk_words);
            if (launch_route(d_args, a.cap_lines, s) != 0) return -1;
        }
        hipLaunchKernelGGL(k_parse_ovf_lines, dim3((unsigned)grid), dim3(PW), lds_ovf, s, a.buf, a.nbytes, d_args,
                           cp.stk_words);
    }
    if (a.mid_event) hipEventRecord((hipEvent_t)a.mid_event, s);
    if (launch_uri(a, d_args, s) != 0) return -1;
    if (launch_geoip(a, d_args, s) != 0) return -1;  // (its status changes reach the counters by atomics)
    // without URI stages the chunks' counts (plus the queued lines' own
    // atomics); with them the URI kernel re-counted every 64-line group
    if (a.uri) return launch_reduce_counts(C.wave_counts, waves, true, C.meta, s);
    return launch_reduce_counts(C.chunk_counts, cp.n_chunks, false, C.meta, s);
}

}  // namespace lp
