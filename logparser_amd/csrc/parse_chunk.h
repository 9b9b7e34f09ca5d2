// The chunked parse kernel (k_parse_chunks / k_parse_deferred) and its wave-level
// pieces, shared by the translation units that instantiate it: parse.hip
// (the instances per program shape class) and parse_fixed.hip (the
// fixed-shape instances, lp_fixed.h), so that make -j compiles them side by
// side.
#pragma once
#include "kernels_common.h"

namespace lp {

namespace {

// ------------------------------------------------------------ chunked parse
// Reference: the caller loop of ApacheHttpdLogfileRecordReader.nextKeyValue
// (ApacheHttpdLogfileRecordReader.java:232-280) reads lines with Hadoop's
// LineRecordReader ('\n', lone '\r' and "\r\n" end a line, the terminator is
// not part of it, a last unterminated line counts; :57, 115) and hands each
// to Parser.parse.  Here the lines of a byte chunk are found by the wave that
// parses them: a line belongs to the chunk holding its first byte.

constexpr int MAXS = PW + 1;
#ifndef LP_CHUNK_MAXW
#define LP_CHUNK_MAXW 10  // waves per CU the chunk plan may size the LDS window for
#endif
#ifndef LP_CHUNK_LMAX
#define LP_CHUNK_LMAX 54  // lines per chunk at most (one-format programs)
#endif
#ifndef LP_MF_WPE
#define LP_MF_WPE 3  // waves per SIMD the several-format chunk instance is compiled for: 3 (168 VGPRs, a few
                     // spilled) measured 10 % faster parse kernels on config 5 than 2 (216 VGPRs), profiles/r06w/mfab
#endif
#ifndef LP_CHUNK_LMAX_MF
#define LP_CHUNK_LMAX_MF 58  // the same for several-format programs (VGPR-bound at 8 waves per CU: 58 measured 6 % faster than 54 on config 5)
#endif  // line starts a chunk keeps in LDS (its 64 lines and the next start)
constexpr uint64_t CS_AGG = 1ull << 62, CS_INC = 1ull << 63, CS_CNT = CS_AGG - 1;

// the line index, written by the chunked parse kernel (read-only elsewhere)
__device__ __forceinline__ LP_G uint64_t* line_off_w(const Columns& C) { return const_cast<LP_G uint64_t*>(C.line_off); }

// Self-checks of the chunked kernels' own bookkeeping.  A failed check is
// counted in Meta::err, the first failure's kind and values kept in
// Meta::err_info, and the batch fails (LP_E_DEVICE, the values on stderr)
// instead of a kernel reading a bad entry:
//   CHK_OVF_LINE  a queued line k_parse_ovf_lines cannot take: q, li, line_off[li], line_off[li + 1]
//   CHK_EXCESS    chunk_excess numbered a different count of lines than the staging pass: c, found, counted, base
//   CHK_QUEUE     a queue append past its capacity: queue (0 lines, 1 chunks), index, entry, capacity
constexpr uint64_t CHK_OVF_LINE = 1, CHK_EXCESS = 2, CHK_QUEUE = 3;
__device__ __forceinline__ void check_fail(const Columns& C, uint64_t kind, uint64_t a, uint64_t b, uint64_t c,
                                           uint64_t d) {
    if (atomicAdd(&C.meta->err, 1ull) == 0) {
        C.meta->err_info[0] = kind;
        C.meta->err_info[1] = a;
        C.meta->err_info[2] = b;
        C.meta->err_info[3] = c;
        C.meta->err_info[4] = d;
    }
}

// Append line li to the queue of k_parse_ovf_lines (cap_lines + 1 entries).
__device__ __forceinline__ void queue_line(const Columns& C, uint64_t li) {
    const uint64_t q = atomicAdd(&C.meta->ovf_lines, 1ull);
    if (q <= (uint64_t)C.cap_lines) C.ovf_lines[q] = (uint32_t)li;
    else check_fail(C, CHK_QUEUE, 0, q, li, (uint64_t)C.cap_lines + 1);
}

// set bits of the wave mask b held by the lanes below this one
__device__ __forceinline__ uint32_t below(uint64_t b) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// What the staging pass of a chunk found: the lines starting in it, the first
// terminator at or after t_hi (the end of its last line), whether the window
// passed the byte guard.
struct ChunkScan {
    uint32_t count;
    uint64_t end_term;  // absolute position, ~0: none in the window
    bool clean;
};

// Stage the window [w0, w1) (w0 64-byte aligned) into LDS with its mask
// planes (two 64-bit planes per 64-byte block, as 16-bit pieces) and find
// the chunk's line starts: every
// terminator t in [t_lo, t_hi) starts a line at t + 1, numbered in order
// from `first` (1 when the chunk also holds the line starting at byte 0).
// starts[r] = window offset of the r-th start (r < MAXS).
//
// The bytes reach LDS by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave
// instruction, no registers held while they are in flight) when the window
// is whole 1 KiB blocks inside the buffer, else (the batch's last chunk) by
// plain loads; then one pass over the LDS copy, a lane taking one whole
// 64-byte mask block per round (bcls::classify64p), makes the two mask planes
// (one 16-byte store per block) and the line terminators: a round is 4 KiB,
// and its starts are ranked once.
__device__ __forceinline__ ChunkScan stage_chunk(const uint8_t* __restrict__ buf, uint64_t nbytes, uint64_t w0,
                                                 uint64_t w1, uint64_t t_lo, uint64_t t_hi, uint32_t first,
                                                 uint8_t* win, uint16_t* msk16, uint32_t* starts) {
    const int lane = lane_id();
    const int nv = (int)((w1 - w0 + 15) >> 4);
    const int nv4 = (nv + 3) & ~3;  // whole 64-byte mask blocks
    if ((nv & (PW - 1)) == 0 && w0 + 16ull * nv <= (nbytes & ~15ull)) {
        for (int k0 = 0; k0 < nv; k0 += PW)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(buf + w0 + 16ull * (k0 + lane)),
                                             (__attribute__((address_space(3))) void*)(win + 16 * k0), 16, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        LP_PROF(63);  // (the window's DMA has landed: the rest of the stage classifies and ranks)
    } else {
        for (int k = lane; k < nv4; k += PW) {
            u32x4 v = u32x4{0, 0, 0, 0};
            if (k < nv) v = load16(buf, nbytes, w0 + 16ull * k);
            *reinterpret_cast<u32x4*>(win + 16 * k) = v;
        }
    }
    // window-relative 32-bit positions (a window is at most 48 KiB); the
    // rounds inside [t_lo, t_hi) and the input (all but the first and the
    // last) skip the boundary masks
    const uint32_t nrel = nbytes - w0 < 16ull * (uint64_t)(nv4 + 1) ? (uint32_t)(nbytes - w0) : 16u * (uint32_t)(nv4 + 1);
    const uint32_t tl = (uint32_t)(t_lo - w0), th = (uint32_t)(t_hi - w0);
    const int nb = nv4 >> 2;     // 64-byte mask blocks: one per lane and round (4 KiB per round)
    uint32_t bad = 0;
    uint32_t run = first;        // starts numbered so far (wave-uniform)
    uint32_t end_rel = ~0u;      // this lane's first terminator >= t_hi (relative)
    u32x4 vn[4];
    LP_UNROLL for (int j = 0; j < 4; ++j)
        vn[j] = lane < nb ? *reinterpret_cast<const u32x4*>(win + 64 * lane + 16 * j) : u32x4{0, 0, 0, 0};
    for (int b0 = 0; b0 < nb; b0 += PW) {  // wave-uniform rounds: every lane joins the ballots
        const int B = b0 + lane;
        const uint32_t q = 64u * (uint32_t)B;
        const uint32_t r0 = 64u * (uint32_t)b0, r1 = r0 + 64u * PW;
        const bool inner = r0 >= tl && r1 <= th && r1 <= nrel && 4 * (b0 + PW) <= nv;  // wave-uniform
        uint64_t tm = 0;
        uint32_t w[16];
        LP_UNROLL for (int j = 0; j < 16; ++j) w[j] = vn[j >> 2][j & 3];
        if (B + PW < nb) {  // the next round's block
            LP_UNROLL for (int j = 0; j < 4; ++j) vn[j] = *reinterpret_cast<const u32x4*>(win + 64 * (B + PW) + 16 * j);
        }
        if (B < nb) {
            bcls::Block64 K = bcls::classify64p(w);
            // the block's planes as msk16 holds them: four u16 of plane 0, then four of plane 1
            *reinterpret_cast<u64x2*>(msk16 + 8 * B) = u64x2{K.p0, K.p1};
            tm = K.lf;
            if (K.other) {  // TAB, '\r' or another control byte (rare): the exact guard and CR terminators
                uint64_t cr = 0;
                LP_UNROLL for (int j = 0; j < 4; ++j) {
                    uint32_t c;
                    bcls::classify16c(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3], K.g[j], c);
                    cr |= (uint64_t)c << (16 * j);
                }
                if (cr) {
                    // "\r\n": the '\n' ends the line; a lone '\r' does (term_bits).  Only a
                    // '\r' in the block's last byte looks past the lane's own registers
                    const uint64_t p = w0 + q;
                    uint64_t next_lf = K.lf >> 1;
                    if ((cr >> 63) && p + 64 < nbytes && buf[p + 64] == '\n') next_lf |= 1ull << 63;
                    tm |= cr & ~next_lf;
                }
            }
            if (inner) {
                bad |= K.g[0] | K.g[1] | K.g[2] | K.g[3];
            } else {
                LP_UNROLL for (int j = 0; j < 4; ++j)
                    if (4 * B + j < nv) bad |= K.g[j];
                if (q + 64 > nrel) tm &= nrel > q ? (1ull << (nrel - q)) - 1ull : 0ull;
            }
        }
        // terminators in [t_lo, t_hi): line starts; the first at or after t_hi: the end
        uint64_t ms = tm;
        if (!inner) {
            uint64_t me = 0;
            if (q < tl) ms &= tl - q >= 64 ? 0ull : ~0ull << (tl - q);
            if (q + 64 > th) {
                const uint64_t lo = th > q ? (1ull << (th - q)) - 1ull : 0ull;
                me = tm & ~lo;
                ms &= lo;
            }
            if (me) end_rel = min(end_rel, q + (uint32_t)__builtin_ctzll(me));
        }
        // rank of this lane's first start in the round: the counts (0..64) of
        // the lanes below it, bit plane by bit plane (ballot + mbcnt; no
        // cross-lane permutes in the loop).  A lane's starts are in position
        // order and the lanes' blocks are, so the round's are in lane order
        const uint32_t c = (uint32_t)__popcll(ms);
        const uint64_t b0m = __ballot(c & 1u), b1m = __ballot(c & 2u);
        uint32_t excl = below(b0m) + 2 * below(b1m);
        uint32_t tot = (uint32_t)(__popcll(b0m) + 2 * __popcll(b1m));
        const uint64_t bh = __ballot(c >= 4u);
        if (bh) {  // wave-uniform: a lane with 4 or more terminators in its 64 bytes (short lines)
            LP_UNROLL for (int k = 2; k < 7; ++k) {
                const uint64_t bk = __ballot(c & (1u << k));
                excl += below(bk) << k;
                tot += (uint32_t)__popcll(bk) << k;
            }
        }
        uint32_t r = run + excl;
        run += tot;
        for (uint64_t m = ms; m; m &= m - 1, ++r)
            if (r < (uint32_t)MAXS) starts[r] = q + (uint32_t)__builtin_ctzll(m) + 1u;
    }
    ChunkScan S;
    S.count = run;
    // wave minimum of the end terminator
    for (int d = 32; d > 0; d >>= 1) end_rel = min(end_rel, (uint32_t)__shfl_xor((int)end_rel, d));
    S.end_term = end_rel == ~0u ? ~0ull : w0 + end_rel;
    S.clean = !__any(bad != 0);
    return S;
}

// The chunks' line numbers.  Chunk c's wave publishes its line count (an
// aggregate) right after staging, without waiting for anything; one scanner
// wave (block 0 of the launch) walks the chunks in order, 512 state words
// per round, and turns every published aggregate into the inclusive prefix;
// chunk c's wave reads its prefix back after phase 1, by when the scanner has
// long passed it.  The scanner only waits for chunks dispatched before the
// ones it has reached, and those publish without waiting, so every wait
// ends.  Each state word is one 8-byte value (status bits and count), stored
// and polled with agent-scope (sc1) accesses: no payload travels beside it.
__device__ __forceinline__ void chunk_publish(LP_G uint64_t* st, int64_t c, uint64_t count) {
    if (lane_id() == 0) __hip_atomic_store(&st[c], CS_AGG | count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __noinline__ void chunk_scanner(LP_G uint64_t* st, int64_t n_chunks) {
    constexpr int PER = 8;  // state words per lane per round
    const int lane = lane_id();
    uint64_t run = 0;
    int64_t c = 0;
    while (c < n_chunks) {
        uint64_t v[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int64_t idx = c + PER * lane + i;
            v[i] = idx < n_chunks ? __hip_atomic_load(&st[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        }
        // this lane's leading published words and their line count
        int pub = 0;
        uint64_t sum = 0;
        bool stop = false;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            stop = stop || !(v[i] & CS_AGG);
            if (!stop) { sum += v[i] & CS_CNT; ++pub; }
        }
        const uint64_t full = __ballot(pub == PER);
        const int L = full == ~0ull ? PW : (int)__builtin_ctzll(~full);  // the first lane with a gap
        const uint64_t mine = lane <= L ? sum : 0ull;
        const uint64_t incl = wave_incl_scan(mine);
        const uint64_t total = __shfl(incl, PW - 1);
        const int pub_L = L < PW ? __shfl(pub, L) : 0;
        if (lane <= L) {
            uint64_t r = run + incl - mine;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                if (i >= pub) break;
                r += v[i] & CS_CNT;
                __hip_atomic_store(&st[c + PER * lane + i], CS_INC | r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const int64_t adv = (int64_t)L * PER + pub_L;
        run += total;
        c += adv;
        if (adv == 0) __builtin_amdgcn_s_sleep(8);
    }
}

// chunk c's first line number (the scanner's prefix minus the chunk's own
// count), or ~0 when the scanner has not reached the chunk after
// CHUNK_WAIT_MAX polls (~10 ms; in a normal launch it has long passed it):
// the wave then leaves the chunk to the deferred pass instead of waiting on,
// so that no wait depends on the order in which the dispatcher starts the
// workgroups (a chunk whose wave was never started cannot hold the others).
// (wait_max: LP_OPT_CHUNK_WAIT, tests; 0 = CHUNK_WAIT_MAX, -1 = defer
// without polling, -2 = defer the odd chunks without polling, the even ones
// as normal: finished and deferred chunks side by side, deterministically)
constexpr uint32_t CHUNK_WAIT_MAX = 1u << 14;
__device__ __forceinline__ uint64_t chunk_base(LP_G uint64_t* st, int64_t c, uint64_t count, int wait_max) {
    if (wait_max < 0 && (wait_max != -2 || (c & 1))) return ~0ull;
    uint64_t v = 0;
    const uint32_t lim = wait_max <= 0 ? CHUNK_WAIT_MAX : (uint32_t)wait_max;
    if (lane_id() == 0) {
        for (uint32_t it = 0;; ++it) {
            v = __hip_atomic_load(&st[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v & CS_INC) break;
            if (it >= lim) { v = ~0ull; break; }
            __builtin_amdgcn_s_sleep(4);
        }
    }
    v = __shfl(v, 0);
    return v == ~0ull ? ~0ull : (v & CS_CNT) - count;
}

// Lines with rank >= 64 in a chunk (more than a wave's lanes): found again
// from the staged window, their line_off entries written and the lines
// queued for k_parse_ovf_lines.  Rare (very short lines).
__device__ __noinline__ void chunk_excess(const uint8_t* __restrict__ buf, uint64_t nbytes, const Columns& C,
                                         const uint8_t* win, uint64_t w0, uint64_t w1, uint64_t t_lo, uint64_t t_hi,
                                         uint32_t first, uint64_t base, int64_t chunk, uint32_t count) {
    const int lane = lane_id();
    const int nv = (int)((w1 - w0 + 15) >> 4);
    uint32_t run = first;
    for (int k0 = 0; k0 < nv; k0 += PW) {
        const int k = k0 + lane;
        const uint64_t p = w0 + 16ull * k;
        uint32_t ms = 0;
        if (k < nv) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(win + 16 * k);
            ms = term_bits(make_uint4(v[0], v[1], v[2], v[3]), buf, p, nbytes);
            if (p < t_lo) ms &= t_lo - p >= 16 ? 0u : ~0u << (uint32_t)(t_lo - p);
            if (p + 16 > t_hi) ms &= t_hi > p ? (1u << (uint32_t)(t_hi - p)) - 1u : 0u;
        }
        const uint32_t c = (uint32_t)__popc(ms);
        const uint32_t incl = wave_incl_scan(c);
        uint32_t r = run + incl - c;
        run += (uint32_t)__shfl((int)incl, 63);
        for (uint32_t m = ms; m; m &= m - 1, ++r) {
            if (r < (uint32_t)PW) continue;
            const uint64_t li = base + r;
            if ((int64_t)li >= C.cap_lines) continue;
            line_off_w(C)[li] = p + (uint64_t)__builtin_ctz(m) + 1;
            queue_line(C, li);
        }
    }
    // the staging pass counted (and published) `count` lines for this chunk
    if (lane == 0 && run != count) {
        check_fail(C, CHK_EXCESS, (uint64_t)chunk, run, count, base);
        if (C.meta->err_info[1] == (uint64_t)chunk) {  // (this chunk's record: the arguments it received)
            C.meta->err_info[5] = w0;
            C.meta->err_info[6] = w1;
            C.meta->err_info[7] = t_lo;
            C.meta->err_info[8] = t_hi;
            C.meta->err_info[9] = first;
            C.meta->err_info[10] = (uint64_t)(uintptr_t)win;
            C.meta->err_info[11] = nbytes;
            C.meta->err_info[12] = (uint64_t)(uintptr_t)buf;
        }
    }
}

// Chunk c of cb bytes on one wave: stage its window, publish its line count,
// phase 1 of its lines, then (its first line number known) the line index
// entries and rows.  LDS: [elements][starts][window (win_cap)]
// [mask planes (win_cap / 4)].  No DFS runs here (a line that needs it is
// queued), so the matchers get a stack without storage (NoStack).
// direct: every line goes to the direct kernel
// (LP_OPT_FORCE_DIRECT, tests).
// second: the deferred pass (the chunk's count is published and the scanner
// has finished: the line number is read, not waited for).
// MF: a program of several LogFormats (HttpdLogFormatDissector.java:173-204):
// each lane first computes its line's match word without the DFS; a line
// that exactly one format matches is routed to it whatever the sticky state
// is (the active format, if it is not that one, fails, and the first that
// matches becomes active), and one that no format matches is BAD whatever
// the state is; so phase 1 runs here for those.  A line several formats
// match, or whose word needs the DFS, is queued: k_route_ovf computes its
// word, the routing scan (k_fmt_*) then gives every line its format, and
// k_parse_ovf_lines parses it.  Every line's word is written to fmt_match.
// SHAPE: the program equals that fixed shape (lp_fixed.h; phase1).
template <bool LA, bool SIMPLE, bool MF = false, int SHAPE = FS_NONE>
__device__ __forceinline__ void parse_chunk(const uint8_t* __restrict__ buf, uint64_t nbytes, const Program& P,
                                            const Columns& C, const Elem* s_elems, uint8_t* smem, int64_t c,
                                            int64_t n_chunks, uint32_t cb, uint32_t win_cap, int direct,
                                            int wait_max, bool second) {
    const uint64_t c0 = (uint64_t)c * cb;
    const uint64_t c1 = c0 + cb < nbytes ? c0 + cb : nbytes;
    const int lane = lane_id();
    const NoStack stk;
    uint32_t* starts = reinterpret_cast<uint32_t*>(smem + 16 * P.n_elems);
    uint8_t* win = smem + 16 * P.n_elems + 16 * ((4 * MAXS + 15) / 16);
    uint16_t* msk16 = reinterpret_cast<uint16_t*>(win + win_cap);
    // window: 64 bytes before the chunk (its first start needs the byte
    // before it), the chunk, then the tail of its last line
    const uint64_t w0 = c0 >= 64 ? c0 - 64 : 0;
    const uint64_t w1 = w0 + win_cap < nbytes ? w0 + win_cap : nbytes;
    const uint64_t t_lo = c0 ? c0 - 1 : 0, t_hi = c1 - 1;
    const uint32_t first = c0 == 0 ? 1u : 0u;
    if (first && lane == 0) starts[0] = 0;
    LP_PROF(0);
    const ChunkScan S = stage_chunk(buf, nbytes, w0, w1, t_lo, t_hi, first, win, msk16, starts);
    if (!second) chunk_publish(C.chunk_state, c, S.count);
    LP_PROF(60);
    __syncthreads();  // starts[] written by every lane
    const uint32_t nl = S.count < (uint32_t)PW ? S.count : (uint32_t)PW;  // lines on this wave's lanes
    const bool has = (uint32_t)lane < nl;
    // this lane's line [s, e) in window offsets; e = its terminator (or end)
    uint32_t s = 0, e = 0;
    bool known = false;
    if (has) {
        s = starts[lane];
        if ((uint32_t)lane + 1 < S.count) {
            e = starts[lane + 1] - 1;
            known = true;
        } else if (S.end_term != ~0ull) {
            e = (uint32_t)(S.end_term - w0);
            known = true;
        } else if (w1 == nbytes) {  // a last line without terminator
            e = (uint32_t)(nbytes - w0);
            known = true;
        }
    }
    const bool lds_line = has && known && !direct;
    const int n = lds_line ? crlf_len((int)(e - s), e > s ? win[e - 1] : 0u) : 0;
    const LineT<lds_bytes, lds_u64> L{(lds_bytes)win, lds_line ? s : 0u, n, (lds_u64)reinterpret_cast<uint64_t*>(msk16)};
    // phase 1 before the line numbers are known (its row is written after)
    LineOut o;
    o.status = ST_OK;
    o.tdone = o.smdone = o.bipdone = 0;
    o.walked = 0;
    LP_PROF(1);
    uint32_t mword = 0;  // MF: the line's match word (bit f: format f matches)
    if constexpr (MF) {
        if (lds_line) {
            bool redo = false;
            // (the spans of the first matching format's first leaf in o.caps)
            mword = fmt_match_word<false>(P, s_elems, L, stk, S.clean, &redo, &o.caps);
            const uint32_t mm = mword & 0xFFu;
            if (redo || (mword >> 8) || (mm & (mm - 1))) o.status = ST_REDO;  // the DFS or the sticky state decides
            else if (mm == 0) o.status = ST_BAD;  // no format matches: BAD in every state
            else phase1<true, LA, false, false, true>(P, s_elems, L, o, stk, C, 0, S.clean, __builtin_ctz(mm));
        }
    } else {
        if (lds_line) phase1<false, LA, SIMPLE, false, false, SHAPE>(P, s_elems, L, o, stk, C, 0, S.clean, 0);  // (no DFS: ST_REDO)
    }
    LP_PROF(9);
    const uint64_t base = chunk_base(C.chunk_state, c, S.count, second ? (int)CHUNK_WAIT_MAX : wait_max);
    if (base == ~0ull) {  // (never in a normal launch) the deferred pass redoes the chunk
        if (lane == 0) {
            const uint64_t q = atomicAdd(&C.meta->deferred, 1ull);
            if (q < (uint64_t)n_chunks) C.deferred_chunks[q] = (uint32_t)c;
            else check_fail(C, CHK_QUEUE, 1, q, (uint64_t)c, (uint64_t)n_chunks);
        }
        return;
    }
    LP_PROF(61);
    const int64_t cap = C.cap_lines;
    const int64_t li = (int64_t)base + lane;
    const bool mine = has && li < cap;
    if (mine) line_off_w(C)[li] = w0 + s;
    if constexpr (MF) {
        if (mine) C.fmt_match[li] = (uint16_t)mword;  // (a queued line's word: k_route_ovf)
    }
    // a line the window does not hold, or that needs the backtracking DFS,
    // is queued for k_parse_ovf_lines (the whole phase 1, from HBM)
    const bool redo = lds_line && o.status == ST_REDO;
    const bool row = mine && lds_line && !redo;
    if (mine && (!lds_line || redo)) queue_line(C, (uint64_t)li);
    {
        const uint32_t nredo = (uint32_t)__popcll(__ballot(mine && redo));
        if (nredo && lane == 0) atomicAdd(&C.meta->dfs_lines, (unsigned long long)nredo);
    }
    if constexpr (SHAPE != FS_NONE) {  // (diagnostic: no atomic for a chunk whose lines all took the straight-line leaf)
        const uint32_t nwalk = (uint32_t)__popcll(__ballot(mine && lds_line && o.walked));
        if (nwalk && lane == 0) atomicAdd(&C.meta->walk_lines, (unsigned long long)nwalk);
    }
    if (row) {
        write_line(P, o, C, li);
        if (!P.has_phase2()) C.arena_base[li] = 0;  // no URI kernel: an empty region for every line
    }
    if (S.count > (uint32_t)PW)
        chunk_excess(buf, nbytes, C, win, w0, w1, t_lo, t_hi, first, base, c, S.count);
    if (c == n_chunks - 1 && lane == 0) {
        // the batch's line count (Hadoop: a last line without terminator counts)
        const uint64_t total = base + S.count;
        C.meta->n_lines = total;
        C.meta->cap_ovf = (int64_t)total > cap ? 1ull : 0ull;
        if ((int64_t)total <= cap) {
            const uint8_t last = buf[nbytes - 1];
            line_off_w(C)[total] = last == '\n' || last == '\r' ? nbytes : nbytes + 1;  // sentinel
        }
    }
    WaveCounts WC;
    WC.act = (uint32_t)__popcll(__ballot(row));
    WC.ok = (uint32_t)__popcll(__ballot(row && o.status == ST_OK));
    WC.bad = (uint32_t)__popcll(__ballot(row && o.status == ST_BAD));
    WC.store(C.chunk_counts, c);
    LP_PROF(62);
}

// Block 0: the scanner; block c + 1: chunk c.  Chunks whose wave stopped
// waiting for the scanner (chunk_base) are redone by k_parse_deferred.
// SIMPLE: the instance for Apache common / combined family programs
// (phase1; the host's simple_program picks it).  SHAPE: the instance of one
// fixed shape (parse_fixed.hip; the host's fixed_shape_of picks it).
template <bool LA, bool SIMPLE, bool MF, int SHAPE = FS_NONE>
__global__ __launch_bounds__(PW, MF ? LP_MF_WPE : 2) void k_parse_chunks(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                     const DeviceArgs* __restrict__ args, uint32_t cb, uint32_t win_cap,
                                                     int direct, int wait_max) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_chunks = (int64_t)((nbytes + cb - 1) / cb);
    if (blockIdx.x == 0) {
        chunk_scanner(C.chunk_state, n_chunks);
        return;
    }
    const int64_t c = (int64_t)blockIdx.x - 1;
    if ((uint64_t)c * cb >= nbytes) return;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Elem* s_elems = reinterpret_cast<Elem*>(smem);
    load_elems(P, s_elems);
    parse_chunk<LA, SIMPLE, MF, SHAPE>(buf, nbytes, P, C, s_elems, smem, c, n_chunks, cb, win_cap, direct, wait_max,
                                       false);
}

// The deferred pass: the chunks in C.deferred_chunks (none in a normal
// launch: its blocks return at once), after k_parse_chunks, whose scanner has
// then finished, so their line numbers are read, not waited for.
template <bool LA, bool SIMPLE, bool MF>
__global__ __launch_bounds__(PW, 2) void k_parse_deferred(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                       const DeviceArgs* __restrict__ args, uint32_t cb,
                                                       uint32_t win_cap, int direct) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const uint64_t nd = C.meta->deferred;
    if (blockIdx.x >= nd) return;
    const int64_t n_chunks = (int64_t)((nbytes + cb - 1) / cb);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Elem* s_elems = reinterpret_cast<Elem*>(smem);
    load_elems(P, s_elems);
    for (uint64_t q = blockIdx.x; q < nd; q += gridDim.x) {
        parse_chunk<LA, SIMPLE, MF>(buf, nbytes, P, C, s_elems, smem, (int64_t)C.deferred_chunks[q], n_chunks, cb,
                                    win_cap, direct, 0, true);
        __syncthreads();  // this chunk's LDS reads are done before the next one is staged
    }
}

}  // namespace
}  // namespace lp
