// gfx950 parse kernels of the logparser_amd engine (phase 1: LogFormat match,
// token flags, time stamps, first line; lp_device.h phase1).
//
//   k_parse_chunks     one-format programs: the line index and phase 1 in ONE pass
//                      over the input.  One wave per byte chunk: the chunk's window
//                      (with the tail of its last line) staged in LDS with its class
//                      masks and line terminators, the lines starting in the chunk
//                      numbered by a decoupled look-back over the chunks' line
//                      counts, one lane per line (the kernel itself: parse_chunk.h,
//                      shared with the fixed-shape instances of parse_fixed.hip)
//   k_parse_ovf_lines  the lines a chunk could not take (more than 64 lines, or a
//                      line ending past its window): read from HBM directly
//   k_parse_lines      several LogFormats: one wave per 64 lines of the line index
//                      (kernels.hip) after the routing pass; the lines' window in LDS
//   k_parse_overflow   the waves k_parse_lines queued (windows LDS cannot hold)
//   k_route_match      several LogFormats: which formats match each line (sticky
//                      routing pass 1)
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
        parse_wave<false>(P, s_elems, C, L, active, li, stk, false, WC);
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

// ------------------------------------------------ line-index parse (several LogFormats)

// One wave's 64 lines on the staged path (k_parse_lines), or queued for
// k_parse_overflow when even half its window exceeds LDS.
__device__ __forceinline__ void parse_group(const uint8_t* __restrict__ buf, uint64_t nbytes, const Program& P,
                                            const Columns& C, const Elem* s_elems, WaveStack stk, uint8_t* win,
                                            uint16_t* msk16, uint32_t win_cap, int64_t wave, int64_t n_lines) {
    const WaveLines W = wave_lines(C, wave, n_lines, nbytes);
    // the lines' window in one staged round; a window larger than LDS in two
    // rounds of 32 lines (lanes 0-31, then 32-63) when each half fits, else
    // the wave is queued for k_parse_overflow (lines read from HBM)
    uint64_t a0 = W.w0, b0 = W.w1, a1 = 0, b1 = 0;
    int rounds = 1;
    if (W.w1 - W.w0 > win_cap) {
        const int64_t mid = W.li0 + PW / 2 < W.lend ? W.li0 + PW / 2 : W.lend;
        const uint64_t lm = C.line_off[mid];
        b0 = lm < nbytes ? lm : nbytes;
        a1 = lm & ~15ull;
        b1 = W.w1;
        rounds = mid < W.lend ? 2 : 1;
        if (b0 - a0 > win_cap || (rounds == 2 && b1 - a1 > win_cap)) {
            if (lane_id() == 0) C.ovf_list[atomicAdd(&C.meta->ovf_waves, 1ull)] = (uint32_t)wave;
            return;
        }
    }
    LP_PROF(0);
    WaveCounts WC;
#pragma nounroll
    for (int r = 0; r < rounds; ++r) {
        const uint64_t a = r ? a1 : a0, b = r ? b1 : b0;
        const bool clean = stage_window(buf, nbytes, a, b, win, msk16);
        __syncthreads();
        const bool mine = W.active && (rounds == 1 || (lane_id() >= PW / 2) == (r != 0));
        const int n = mine ? crlf_len(W.n, W.n > 0 ? win[W.e - 1 - a] : 0u) : 0;
        const LineT<lds_bytes, lds_u64> L{(lds_bytes)win, mine ? (uint32_t)(W.s - a) : 0u, n,
                                          (lds_u64)reinterpret_cast<uint64_t*>(msk16)};
        parse_wave<true>(P, s_elems, C, L, mine, W.li, stk, clean, WC);
        if (r + 1 < rounds) __syncthreads();  // this round's LDS reads are done before the next staging
    }
    WC.store(C, wave);
}

__global__ __launch_bounds__(PW, 2) void k_parse_lines(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                    const DeviceArgs* __restrict__ args, uint32_t win_cap,
                                                    uint32_t stk_words) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_lines = (int64_t)C.meta->n_lines;
    const int64_t wave = blockIdx.x;
    if (wave * PW >= n_lines || C.meta->cap_ovf) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Elem* s_elems = reinterpret_cast<Elem*>(smem);
    WaveStack stk{reinterpret_cast<uint32_t*>(smem + 16 * P.n_elems) + lane_id()};
    uint8_t* win = smem + 16 * P.n_elems + stk_words * 4;
    uint16_t* msk16 = reinterpret_cast<uint16_t*>(win + win_cap);
    load_elems(P, s_elems);
    parse_group(buf, nbytes, P, C, s_elems, stk, win, msk16, win_cap, wave, n_lines);
}

// The waves k_parse_lines queued (even half their window exceeds LDS: very
// long lines), on a persistent grid: the lines are read from HBM directly.
__global__ __launch_bounds__(PW) void k_parse_overflow(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                       const DeviceArgs* __restrict__ args, uint32_t stk_words) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_lines = (int64_t)C.meta->n_lines;
    const uint64_t nq = C.meta->ovf_waves;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Elem* s_elems = reinterpret_cast<Elem*>(smem);
    WaveStack stk{reinterpret_cast<uint32_t*>(smem + 16 * P.n_elems) + lane_id()};
    load_elems(P, s_elems);
    __syncthreads();
    for (uint64_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const int64_t wave = C.ovf_list[q];
        const WaveLines W = wave_lines(C, wave, n_lines, nbytes);
        WaveCounts WC;
        // base = the line start aligned down to 4 bytes: word reads never
        // leave the 4-byte words holding the line's bytes
        const LP_G uint8_t* ls = (const LP_G uint8_t*)(buf) + W.s;
        const uint32_t mis = (uint32_t)((uintptr_t)ls & 3);
        const LineT<const LP_G uint8_t*> L{ls - mis, mis, crlf_len_hbm(buf, W)};
        parse_wave<true>(P, s_elems, C, L, W.active, W.li, stk, false, WC);
        __syncthreads();
        WC.store(C, wave);
    }
}

// Sticky routing pass 1: the match word of every line (bit f = format f matches).
__global__ __launch_bounds__(PW) void k_route_match(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                    const DeviceArgs* __restrict__ args, uint32_t win_cap,
                                                    uint32_t stk_words) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_lines = (int64_t)C.meta->n_lines;
    const int64_t wave = blockIdx.x;
    if (wave * PW >= n_lines || C.meta->cap_ovf) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Elem* s_elems = reinterpret_cast<Elem*>(smem);
    WaveStack stk{reinterpret_cast<uint32_t*>(smem + 16 * P.n_elems) + lane_id()};
    uint8_t* win = smem + 16 * P.n_elems + stk_words * 4;
    uint16_t* msk16 = reinterpret_cast<uint16_t*>(win + win_cap);
    load_elems(P, s_elems);
    const WaveLines W = wave_lines(C, wave, n_lines, nbytes);
    if (W.w1 - W.w0 <= win_cap) {
        const bool clean = stage_window(buf, nbytes, W.w0, W.w1, win, msk16);
        __syncthreads();
        const int n = W.active ? crlf_len(W.n, W.n > 0 ? win[W.e - 1 - W.w0] : 0u) : W.n;
        const LineT<lds_bytes, lds_u64> L{(lds_bytes)win, (uint32_t)(W.s - W.w0), n, (lds_u64)reinterpret_cast<uint64_t*>(msk16)};
        if (W.active) C.fmt_match[W.li] = (uint16_t)fmt_match_word(P, s_elems, L, stk, clean);
    } else {
        __syncthreads();
        const LP_G uint8_t* ls = (const LP_G uint8_t*)(buf) + W.s;
        const uint32_t mis = (uint32_t)((uintptr_t)ls & 3);
        const LineT<const LP_G uint8_t*> L{ls - mis, mis, crlf_len_hbm(buf, W)};
        if (W.active) C.fmt_match[W.li] = (uint16_t)fmt_match_word(P, s_elems, L, stk, false);
    }
}

// LDS window of a wave: sized to the most waves per CU that still leave >= 4 %
// over the mean 64 lines (the few windows that do not fit go to the direct
// kernel).  Measured on gfx950: W waves of one 64-thread workgroup each fit
// when a wave's LDS is at most 160 KiB / W - 640 B.
struct WindowPlan {
    uint32_t cap, stk_words;
    size_t lds;
};
WindowPlan window_plan(const ParseLaunch& a) {
    WindowPlan w;
    w.stk_words = (uint32_t)(a.stack_depth > 0 ? a.stack_depth : 1) * PW;
    const uint64_t fixed = 16 * (uint64_t)a.n_elems + 4 * (uint64_t)w.stk_words;
    const uint64_t per8 = 8 + MC_N;  // LDS bytes per 8 window bytes (window + mask planes)
    const uint64_t mean = a.mean_line ? a.mean_line : 256;
    const uint64_t need = PW * mean + PW * mean / 25 + 64;
    uint64_t cap = 0;
    for (int k = 8; k >= 2 && !cap; --k) {
        const uint64_t budget = 160 * 1024 / k - 640;
        if (budget <= fixed) continue;
        const uint64_t c = ((budget - fixed) * 8 / per8) & ~63ull;
        if (c >= need) cap = c;
    }
    if (!cap) cap = ((PW * mean * 110) / 100 + 512 + 63) & ~63ull;
    if (cap > 48 * 1024) cap = 48 * 1024;
    if (a.force_direct) cap = 0;
    w.cap = (uint32_t)cap;
    w.lds = fixed + cap + MC_N * (cap / 8);
    return w;
}

}  // namespace

// The chunked kernel's LDS: a window of the most waves per CU that still
// holds the chunk (target_lines x the mean line) plus 64 bytes before it and
// an overhang of at least 2 mean lines for the tail of its last line.
ChunkPlan chunk_plan(const ParseLaunch& a) {
    ChunkPlan c{};
    c.stk_words = (uint32_t)(a.stack_depth > 0 ? a.stack_depth : 1) * PW;
    // the chunk kernels run no DFS (ST_REDO lines are queued): no stack in
    // their LDS (the queued lines' kernels have theirs)
#if defined(LP_DFS_IN_CHUNKS)
    c.chunk_stk = c.stk_words;
#else
    c.chunk_stk = 0;
#endif
    const uint64_t fixed = 16 * (uint64_t)a.n_elems + 4 * (uint64_t)c.chunk_stk + 16 * ((4 * MAXS + 15) / 16);
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

int launch_route_match(const ParseLaunch& a, const DeviceArgs* d_args, hipStream_t s) {
    const int64_t waves = parse_waves(a.cap_lines);
    if (waves == 0) return 0;
    const WindowPlan w = window_plan(a);
    hipLaunchKernelGGL(k_route_match, dim3((unsigned)waves), dim3(PW), w.lds, s, a.buf, a.nbytes, d_args, w.cap,
                       w.stk_words);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_parse(const ParseLaunch& a, const DeviceArgs* d_args, const Columns& C, hipStream_t s) {
    const int64_t waves = parse_waves(a.cap_lines);
    if (waves == 0 && !a.chunked) {
        if (a.mid_event) hipEventRecord((hipEvent_t)a.mid_event, s);
        return 0;
    }
    const int64_t grid = std::max<int64_t>(1, waves < 1024 ? waves : 1024);
    if (a.chunked) {
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
                hipLaunchKernelGGL(chunks, dim3(g0), dim3(PW), cp.lds, s, a.buf, a.nbytes, d_args, cp.cb, cp.win_cap,
                                   cp.chunk_stk, fd, a.chunk_wait);
                hipLaunchKernelGGL(deferred, dim3(g1), dim3(PW), cp.lds, s, a.buf, a.nbytes, d_args, cp.cb,
                                   cp.win_cap, cp.chunk_stk, fd);
            };
#if defined(LP_NO_SIMPLE)  // (experiment builds: every program on the general instances)
            const bool simple = false;
#else
            const bool simple = a.simple;
#endif
            // (several LogFormats: one instance; their first leaves are walked per lane)
            // (a fixed shape: its own chunk instance, the SIMPLE deferred pass)
            if (a.shape != FS_NONE && !a.multi && !a.lit_aware && simple) {
                if (launch_chunks_fixed(a, d_args, cp, g0, s) != 0) return -1;
                hipLaunchKernelGGL((k_parse_deferred<false, true, false>), dim3(g1), dim3(PW), cp.lds, s, a.buf,
                                   a.nbytes, d_args, cp.cb, cp.win_cap, cp.chunk_stk, fd);
            } else if (a.multi) run(k_parse_chunks<true, false, true>, k_parse_deferred<true, false, true>);
            else if (a.lit_aware && simple) run(k_parse_chunks<true, true, false>, k_parse_deferred<true, true, false>);
            else if (a.lit_aware) run(k_parse_chunks<true, false, false>, k_parse_deferred<true, false, false>);
            else if (simple) run(k_parse_chunks<false, true, false>, k_parse_deferred<false, true, false>);
            else run(k_parse_chunks<false, false, false>, k_parse_deferred<false, false, false>);
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
        // without URI stages the chunks' counts (plus the queued lines' own
        // atomics); with them the URI kernel re-counted every 64-line group
        if (a.uri) return launch_reduce_counts(C.wave_counts, waves, true, C.meta, s);
        return launch_reduce_counts(C.chunk_counts, cp.n_chunks, false, C.meta, s);
    }
    const WindowPlan w = window_plan(a);
    hipLaunchKernelGGL(k_parse_lines, dim3((unsigned)waves), dim3(PW), w.lds, s, a.buf, a.nbytes, d_args, w.cap,
                       w.stk_words);
    // the queued waves (even half the window exceeds LDS): persistent grid,
    // lines read from HBM (LDS: the elements and the DFS stack only)
    const size_t lds_ovf = 16 * (size_t)a.n_elems + 4 * (size_t)w.stk_words;
    hipLaunchKernelGGL(k_parse_overflow, dim3((unsigned)grid), dim3(PW), lds_ovf, s, a.buf, a.nbytes, d_args,
                       w.stk_words);
    if (a.mid_event) hipEventRecord((hipEvent_t)a.mid_event, s);
    if (launch_uri(a, d_args, s) != 0) return -1;
    return launch_reduce_counts(C.wave_counts, waves, true, C.meta, s);
}

}  // namespace lp
