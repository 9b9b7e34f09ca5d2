// gfx950 kernels of the device table: lp_result_table on a device view
// (include/logparser_amd.h), the ParsedRecord / Hive SerDe output side
// (httpdlog-inputformat/.../ParsedRecord.java:154-214: set(name, value), a
// null ignored, the last value wins; httpdlog-serde/.../ApacheHttpdlogDeserializer.java:
// 224-240, 295-323: STRING / BIGINT / DOUBLE columns, one row per line) built
// from the parse kernels' SoA columns without leaving HBM:
//
//   k_table_values  one lane per row: each column's value from the source the
//                   planner named (lp_table.h), the validity byte, LONG /
//                   DOUBLE values, and each STRING value's length and where
//                   its bytes are (TableArgs::srcw)
//   (scan)          the lengths -> Arrow offsets (hipCUB inclusive sum)
//   k_table_chars   one wave per 64 rows of a STRING column: the column's
//                   bytes of those rows, written 4-byte word by word
//
// What each source delivers mirrors Plan::replay (plan.cpp) case by case.
//
// Row lists (lp_result_table_rows / lp_result_table_map_rows: the dense
// tables of the lines a record reader keeps, ApacheHttpdLogfileRecordReader.java:
// 246-287, ApacheHttpdlogDeserializer.java:284-291): the kernels that turn a row
// into a line have a second instance (EXT) that takes the line from
// TableArgs::rows / MapArgs::rows, bound-checked, and evaluates the
// pseudo-columns (lp_table.h TC_LINE..TC_STATUS).  The contiguous instances
// are the code they were before the row lists.
#include <hip/hip_runtime.h>

#define LP_KERNEL_TU 1  // device column pointers are global-memory pointers (lp_program.h)

#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "lp_device.h"
#include "table_value.h"  // TVal, tvalue, row_view, row_line

namespace lp {

namespace {

constexpr int TB = 256;

template <bool EXT, bool GEO>
__global__ __launch_bounds__(TB) void k_table_values(const DeviceArgs* __restrict__ args,
                                                     const TableArgs* __restrict__ targs, const uint8_t* buf) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const TableArgs& T = *targs;
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= T.count) return;
    int64_t i = T.first + k;
    bool in_batch = true;
    if constexpr (EXT) in_batch = row_line(T.rows, T.first, T.n_lines, T.bad_row, k, i);
    const LP_G uint8_t *line = nullptr, *region = nullptr;
    const bool ok = in_batch && row_view(P, C, buf, i, line, region);
    const int fmt = ok && P.n_fmt > 1 ? (int)C.fmt_id[i] : 0;
    for (int c = 0, rank = 0; c < T.n_cols; ++c) {
        const TableCol& col = T.cols[c];
        bool valid = false;
        int64_t x = 0;
        double d = 0.0;
        uint64_t w = 0;
        if constexpr (EXT) {
            // a pseudo-column: before the status test, valid for every row of the batch
            const int32_t pk = col.src[0].kind;
            if (in_batch && tc_pseudo(pk)) {
                if (pk == TC_LINE) {  // the parse kernels' line: wave_lines' end, crlf_len
                    const uint64_t s0 = C.line_off[i], e0 = C.line_off[i + 1] - 1;
                    const LP_G uint8_t* lp = (const LP_G uint8_t*)buf + s0;
                    uint64_t n = e0 - s0;
                    if (n > 0 && lp[n - 1] == '\r') --n;
                    x = (int64_t)n;
                    w = (uint64_t)(uintptr_t)lp;
                    valid = col.kind == 1;
                } else {
                    x = pk == TC_OFFSET ? (int64_t)C.line_off[i] : pk == TC_LINENO ? T.first_line + i : (int64_t)C.status[i];
                    valid = col.kind == 2;
                }
            }
        }
        // the later delivery, then (a value that is none for the column) the earlier
        for (int pass = 0; pass < 2 && ok && !valid; ++pass) {
            const TableSrc& sc = pass ? col.alt[fmt] : col.src[fmt];
            if (pass && sc.kind == TC_NONE) break;
            const TVal v = tvalue_any<GEO>(P, C, T, sc, i, line, region);
            valid = v.kind != 0;
            if (col.kind == 1) {  // STRING: its length now, its bytes after the scan
                x = v.kind == 2 ? digits(v.l) : v.n + (v.amp ? 1u : 0u);
                // where k_table_chars finds them (lp_table.h SW_*)
                const uint64_t pa = (uint64_t)(uintptr_t)v.p;
                if (v.kind == 1 && pa < SW_AMP) w = pa | (v.amp ? SW_AMP : 0ull);
                else if (v.kind == 2 && v.l >= -(int64_t)SW_AMP && v.l < (int64_t)SW_AMP)
                    w = SW_LONG | ((uint64_t)v.l & (SW_LONG - 1));
                else w = SW_SLOW;
            } else if (col.kind == 2) {
                x = v.l;
                if (v.kind == 1) valid = parse_long(v.p, v.n, v.amp, x);
                else if (v.kind == 3) valid = false;  // month names, dates: not numbers
            } else {
                // the planner admits long-valued sources and SECOND_MILLIS list items here
                if (v.kind == 1 && sc.kind == TC_LIST) d = decimal_to_double(v.p, v.n);
                else if (v.kind == 2) d = (double)v.l;
                else valid = false;
                if constexpr (GEO)  // a DOUBLE field: its text, the f64's bits in l
                    if (v.kind == 1 && sc.kind == TC_GEOIP && sc.c == GK_DOUBLE) { d = __longlong_as_double(v.l); valid = true; }
            }
        }
        if (col.kind == 1) {
            col.i64[k + 1] = valid ? x : 0;
            if (k == 0) col.i64[0] = 0;
            T.srcw[(int64_t)rank++ * T.count + k] = valid ? w : 0;
        } else if (col.kind == 2) {
            if (valid) col.i64[k] = x;
        } else if (valid) {
            col.f64[k] = d;
        }
        col.valid[k] = valid ? 1 : 0;
    }
}

// The STRING columns' bytes, destination-major: one wave per 64 rows of one
// STRING column (grid y = the column's rank among the STRING columns).  The
// wave's rows fill one contiguous byte range of the column ([off[k0],
// off[k0 + 64]), Arrow offsets), so the wave walks that range 256 bytes per
// step, lane l on its 4-byte word: each byte's row by a binary search over
// the rows' offsets in LDS, its source byte from the input / arena (a value's
// bytes), the wave's LDS scratch (formatted longs, dates, binary IPs) or the
// '&' of a raw query string, and one aligned 4-byte store per full word
// (byte stores only at the range's two ends, whose words the neighbouring
// waves share).  Consecutive lanes read consecutive source bytes of a row and
// write consecutive words: the traffic is coalesced both ways.
constexpr int CW = 4;    // waves per block
constexpr int FMTB = 24; // scratch bytes per row (a long's 20 characters at most)

template <bool EXT>
__global__ __launch_bounds__(64 * CW) void k_table_chars(const DeviceArgs* __restrict__ args,
                                                         const TableArgs* __restrict__ targs, const uint8_t* buf) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const TableArgs& T = *targs;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ uint32_t s_off[CW][65];
    __shared__ uint32_t s_flag[CW][64];
    __shared__ uint64_t s_src[CW][64];
    __shared__ uint8_t s_fmt[CW][64 * FMTB];
    // the column: the blockIdx.y-th STRING column
    int c = -1;
    for (int j = 0, r = 0; j < T.n_cols; ++j)
        if (T.cols[j].kind == 1 && r++ == (int)blockIdx.y) c = j;
    const int64_t k0 = ((int64_t)blockIdx.x * CW + wv) * 64;
    if (c < 0 || k0 >= T.count) return;  // wave-uniform; only wave-level LDS sharing below
    const TableCol& col = T.cols[c];
    const int64_t kend = k0 + 64 < T.count ? k0 + 64 : T.count;
    const int nrows = (int)(kend - k0);
    const int64_t k = k0 + lane;
    const uint64_t D0 = (uint64_t)col.i64[k0], D1 = (uint64_t)col.i64[kend];
    uint32_t flag = 0;  // bit 0: bytes in the scratch; bit 1: a leading '&'
    uint64_t src = 0;
    // the row's value as k_table_values found it (one coalesced word: no
    // status -> line -> span chain here); a long is formatted into the wave's
    // scratch, a SW_SLOW value derived again
    const uint64_t w = k < kend ? T.srcw[(int64_t)blockIdx.y * T.count + k] : 0;
    if (k < kend && col.valid[k]) {
        uint8_t* f = &s_fmt[wv][lane * FMTB];
        TVal v;
        if ((w >> 62) == 0) {
            v.kind = 1;
            v.p = reinterpret_cast<const LP_G uint8_t*>((uintptr_t)(w & (SW_AMP - 1)));
            v.amp = (w & SW_AMP) != 0;
        } else if ((w >> 62) == 1) {
            v.kind = 2;
            v.l = (int64_t)(w << 2) >> 2;
        } else {
            const LP_G uint8_t *line = nullptr, *region = nullptr;
            int64_t i = T.first + k;
            bool in_batch = true;  // (a valid row's line is inside the batch: k_table_values checked it)
            if constexpr (EXT) in_batch = row_line(T.rows, T.first, T.n_lines, T.bad_row, k, i);
            if (in_batch && row_view(P, C, buf, i, line, region)) {
                const int fmt = P.n_fmt > 1 ? (int)C.fmt_id[i] : 0;
                v = tvalue(P, C, T, col.src[fmt], i, line, region);
                if (v.kind == 0) v = tvalue(P, C, T, col.alt[fmt], i, line, region);  // the earlier delivery
            }
        }
        if (v.kind == 2) {
            write_long(f, v.l, digits(v.l));
            flag = 1;
        } else if (v.kind == 3) {
            for (uint32_t q = 0; q < v.n; ++q) f[q] = (uint8_t)v.buf[q];
            flag = 1;
        } else {
            src = (uint64_t)(uintptr_t)v.p;
            flag = v.amp ? 2u : 0u;
        }
    }
    if (lane < nrows) {
        s_off[wv][lane] = (uint32_t)((uint64_t)col.i64[k] - D0);
        s_flag[wv][lane] = flag;
        s_src[wv][lane] = src;
    }
    if (lane == 0) s_off[wv][nrows] = (uint32_t)(D1 - D0);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (D1 == D0) return;
    const uint32_t total = (uint32_t)(D1 - D0);
    const uint32_t* off = s_off[wv];
    // 4-byte words of the destination: offsets congruent to -mis mod 4
    const uint32_t mis = (uint32_t)((uintptr_t)col.chars & 3u);
    const uint64_t A0 = D0 - ((D0 + mis) & 3u);
    LP_G uint8_t* const out = col.chars;
    // U words per lane per step: every source byte load of the step is in
    // flight before the first store
    constexpr int U = 4;
    for (uint64_t a0 = A0; a0 < D1; a0 += 256 * U) {
        uint32_t word[U], have[U];
        uint8_t bv[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t d = a0 + 256ull * u + 4ull * (uint64_t)lane;
            have[u] = 0;
            if (!(d < D1 && d + 4 > D0)) continue;
            const uint32_t t0 = d < D0 ? (uint32_t)(D0 - d) : 0u;
            const uint32_t x0 = (uint32_t)(d + t0 - D0);  // the first byte in range, relative
            int r = 0;
            for (int st = 32; st; st >>= 1)
                if (r + st < nrows && off[r + st] <= x0) r += st;
            uint32_t nxt = off[r + 1], beg = off[r], fl = s_flag[wv][r];
            uint64_t sp = s_src[wv][r];
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const uint32_t x = x0 + t - t0;
                if (t < t0 || x >= total) continue;
                while (x >= nxt) {  // the next non-empty row
                    ++r;
                    beg = nxt;
                    nxt = off[r + 1];
                    fl = s_flag[wv][r];
                    sp = s_src[wv][r];
                }
                const uint32_t o = x - beg;
                if (fl & 1u) bv[u][t] = s_fmt[wv][r * FMTB + o];
                else if ((fl & 2u) && o == 0) bv[u][t] = '&';
                else bv[u][t] = reinterpret_cast<const LP_G uint8_t*>((uintptr_t)sp)[o - (fl >> 1)];
                have[u] |= 1u << t;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t d = a0 + 256ull * u + 4ull * (uint64_t)lane;
            word[u] = 0;
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t)
                if ((have[u] >> t) & 1u) word[u] |= (uint32_t)bv[u][t] << (8 * t);
            if (have[u] == 15u) {
                *reinterpret_cast<LP_G uint32_t*>(out + d) = word[u];
            } else if (have[u]) {
                for (uint32_t t = 0; t < 4; ++t)
                    if ((have[u] >> t) & 1u) out[d + t] = (uint8_t)(word[u] >> (8 * t));
            }
        }
    }
}

// ---- map columns (lp_result_table_map on a device view): a wildcard target
// "TYPE:prefix.*" as an Arrow map<string,string> per row -- ParsedRecord's
// setMultiValueString (httpdlog-inputformat/.../ParsedRecord.java:178-196: the
// key is the name after the prefix, a null is ignored, a later value of a key
// replaces the earlier) over the piece table of the query / pair stage that
// delivers the wildcard's members (lp_table.h MapArgs):
//
//   k_map_count    one lane per row: the validity byte, the row's piece count
//   (scan)         the counts -> piece bases
//   k_map_entries  one lane per PIECE (a 300-piece line is 300 lanes, not one):
//                  its row by a binary search over the piece bases; it
//                  survives when its name was requested and no later piece of
//                  the row has the same name; key / value lengths and where
//                  their bytes are (SW_PTR words: names and values are refs)
//   (scans)        the survive flags -> entry indices; the lengths -> offsets
//   k_map_fill     entry_off per row, key_off / val_off and the source words
//                  per surviving piece, compacted to its entry
//   k_map_chars    one wave per 64 entries of the keys (grid y 0) or values
//                  (1): k_table_chars' destination-major walk
//
// An entry stands at the position of its key's last piece: the order the host
// replay (capi.cpp) produces too.

// the row's piece table of the column's source (null: none)
__device__ __forceinline__ const LP_G uint64_t* map_table(const Program& P, const Columns& C, const MapArgs& M, int64_t i,
                                                          const LP_G uint8_t* region) {
    const MapSrc s = M.src[P.n_fmt > 1 ? (int)C.fmt_id[i] : 0];
    if (s.kind == MS_QUERY) return reinterpret_cast<const LP_G uint64_t*>(region + ref_off(C.q_params[s.a][i]));
    if (s.kind == MS_PAIR) return reinterpret_cast<const LP_G uint64_t*>(region + ref_off(C.p_tab[s.a][i]));
    return nullptr;
}

template <bool EXT>
__global__ __launch_bounds__(TB) void k_map_count(const DeviceArgs* __restrict__ args, const MapArgs M) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k > M.count) return;
    if (k == M.count) { M.cnt[k] = 0; return; }  // the scan's last item: the piece total
    int64_t i = M.first + k;
    bool in_batch = true;
    if constexpr (EXT) in_batch = row_line(M.rows, M.first, M.n_lines, M.bad_row, k, i);
    const bool ok = in_batch && C.status[i] == ST_OK;
    int64_t n = 0;
    if (ok) {
        const MapSrc s = M.src[P.n_fmt > 1 ? (int)C.fmt_id[i] : 0];
        if (s.kind == MS_QUERY) n = C.q_count[s.a][i];
        else if (s.kind == MS_PAIR) n = C.p_count[s.a][i];
    }
    M.valid[k] = ok ? 1 : 0;  // an OK line has a record: its map may be empty
    M.cnt[k] = n;
}

template <bool EXT>
__global__ __launch_bounds__(TB) void k_map_entries(const DeviceArgs* __restrict__ args, const MapArgs M,
                                                    const uint8_t* buf) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t p = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (p > M.n_pieces) return;
    if (p == M.n_pieces) {  // the scans' last item: the totals
        M.flag[p] = 0;
        M.klen[p] = 0;
        M.vlen[p] = 0;
        return;
    }
    // the piece's row: the last one whose base is <= p (pbase[count] = n_pieces > p; a row
    // without pieces shares its base with the next)
    int64_t lo = 0, hi = M.count;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (M.pbase[mid] <= p) lo = mid;
        else hi = mid;
    }
    // (a row with pieces passed k_map_count's bound check: its line is inside the batch)
    const int64_t i = EXT ? M.rows[lo] : M.first + lo;
    const uint32_t j = (uint32_t)(p - M.pbase[lo]), cnt = (uint32_t)(M.pbase[lo + 1] - M.pbase[lo]);
    const LP_G uint8_t *line = nullptr, *region = nullptr;
    row_view(P, C, buf, i, line, region);  // (a row with pieces is OK)
    const LP_G uint64_t* t = map_table(P, C, M, i, region);
    const uint64_t nref = t[2 * j], vref = t[2 * j + 1];
    const uint32_t nlen = ref_len(nref);
    const LP_G uint8_t* np = (ref_arena(nref) ? region : line) + ref_off(nref);
    bool live = nref != REF_SKIP;  // a name that was not requested delivers nothing
    for (uint32_t q = j + 1; q < cnt && live; ++q) {
        const uint64_t n2 = t[2 * q];
        if (n2 == REF_SKIP || ref_len(n2) != nlen) continue;
        const LP_G uint8_t* p2 = (ref_arena(n2) ? region : line) + ref_off(n2);
        bool same = true;
        for (uint32_t b = 0; b < nlen && same; ++b) same = np[b] == p2[b];
        live = !same;  // a later value of the key replaces this one
    }
    const uint64_t vp = (uint64_t)(uintptr_t)((ref_arena(vref) ? region : line) + ref_off(vref));
    M.flag[p] = live ? 1u : 0u;
    M.klen[p] = live ? (int64_t)nlen : 0;
    M.vlen[p] = live ? (int64_t)ref_len(vref) + (ref_amp(vref) ? 1 : 0) : 0;
    M.ksrc[p] = (uint64_t)(uintptr_t)np;
    M.vsrc[p] = vp | (ref_amp(vref) ? SW_AMP : 0ull);
}

__global__ __launch_bounds__(TB) void k_map_fill(const MapArgs M) {
    const int64_t t = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (t <= M.count) M.entry_off[t] = (int64_t)M.eidx[M.pbase[t]];
    if (t > M.n_pieces) return;
    const uint32_t e = M.eidx[t];
    if (t == M.n_pieces || M.flag[t]) {  // an entry's start; the last item: the ends of the last entry
        M.key_off[e] = M.kpos[t];
        M.val_off[e] = M.vpos[t];
    }
    if (t < M.n_pieces && M.flag[t]) {
        M.ksrc_e[e] = M.ksrc[t];
        M.vsrc_e[e] = M.vsrc[t];
    }
}

// The keys' (blockIdx.y 0) or values' (1) bytes, destination-major: one wave
// per 64 entries, k_table_chars' walk with every value a SW_PTR word.
__global__ __launch_bounds__(64 * CW) void k_map_chars(const MapArgs M, int64_t n_entries) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ uint32_t s_off[CW][65];
    __shared__ uint64_t s_src[CW][64];
    const bool keys = blockIdx.y == 0;
    const LP_G int64_t* const eoff = keys ? M.key_off : M.val_off;
    const LP_G uint64_t* const esrc = keys ? M.ksrc_e : M.vsrc_e;
    LP_G uint8_t* const out = keys ? M.key_chars : M.val_chars;
    const int64_t k0 = ((int64_t)blockIdx.x * CW + wv) * 64;
    if (k0 >= n_entries) return;  // wave-uniform; only wave-level LDS sharing below
    const int64_t kend = k0 + 64 < n_entries ? k0 + 64 : n_entries;
    const int nrows = (int)(kend - k0);
    const int64_t k = k0 + lane;
    const uint64_t D0 = (uint64_t)eoff[k0], D1 = (uint64_t)eoff[kend];
    if (lane < nrows) {
        s_off[wv][lane] = (uint32_t)((uint64_t)eoff[k] - D0);
        s_src[wv][lane] = esrc[k];
    }
    if (lane == 0) s_off[wv][nrows] = (uint32_t)(D1 - D0);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (D1 == D0) return;
    const uint32_t total = (uint32_t)(D1 - D0);
    const uint32_t* off = s_off[wv];
    // 4-byte words of the destination: offsets congruent to -mis mod 4
    const uint32_t mis = (uint32_t)((uintptr_t)out & 3u);
    const uint64_t A0 = D0 - ((D0 + mis) & 3u);
    constexpr int U = 4;  // words per lane per step: the step's loads in flight before its first store
    for (uint64_t a0 = A0; a0 < D1; a0 += 256 * U) {
        uint32_t word[U], have[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t d = a0 + 256ull * u + 4ull * (uint64_t)lane;
            have[u] = 0;
            word[u] = 0;
            if (!(d < D1 && d + 4 > D0)) continue;
            const uint32_t t0 = d < D0 ? (uint32_t)(D0 - d) : 0u;
            const uint32_t x0 = (uint32_t)(d + t0 - D0);  // the first byte in range, relative
            int r = 0;
            for (int st = 32; st; st >>= 1)
                if (r + st < nrows && off[r + st] <= x0) r += st;
            uint32_t nxt = off[r + 1], beg = off[r];
            uint64_t sp = s_src[wv][r];
#pragma unroll
            for (uint32_t t = 0; t < 4; ++t) {
                const uint32_t x = x0 + t - t0;
                if (t < t0 || x >= total) continue;
                while (x >= nxt) {  // the next non-empty entry
                    ++r;
                    beg = nxt;
                    nxt = off[r + 1];
                    sp = s_src[wv][r];
                }
                const uint32_t o = x - beg, amp = (sp & SW_AMP) ? 1u : 0u;
                const uint8_t b = amp && o == 0
                                      ? (uint8_t)'&'
                                      : reinterpret_cast<const LP_G uint8_t*>((uintptr_t)(sp & (SW_AMP - 1)))[o - amp];
                word[u] |= (uint32_t)b << (8 * t);
                have[u] |= 1u << t;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t d = a0 + 256ull * u + 4ull * (uint64_t)lane;
            if (have[u] == 15u) {
                *reinterpret_cast<LP_G uint32_t*>(out + d) = word[u];
            } else if (have[u]) {
                for (uint32_t t = 0; t < 4; ++t)
                    if ((have[u] >> t) & 1u) out[d + t] = (uint8_t)(word[u] >> (8 * t));
            }
        }
    }
}

}  // namespace

// scratch: the scan's temporary storage, its sums, the STRING value words
size_t table_srcw_offset(int64_t count) {
    size_t tmp = 0;
    hipcub::DeviceScan::InclusiveSum(nullptr, tmp, (const int64_t*)nullptr, (int64_t*)nullptr, (int)count);
    return ((tmp + 255) & ~(size_t)255) + ((8 * (size_t)count + 255) & ~(size_t)255);
}

size_t table_scratch_bytes(int64_t count, int n_str) {
    return table_srcw_offset(count) + 8 * (size_t)count * (size_t)n_str + 256;
}

// the row-list instances: a row list, or a pseudo-column (the same for every LogFormat)
bool table_ext(const TableArgs& ta) {
    if (ta.rows) return true;
    for (int c = 0; c < ta.n_cols; ++c)
        if (tc_pseudo(ta.cols[c].src[0].kind)) return true;
    return false;
}

int launch_table_values(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const uint8_t* buf,
                        void* scratch, size_t scratch_bytes, hipStream_t s, hipEvent_t mid, bool offsets) {
    if (ta.count > 0x7FFFFFFF) return -1;  // the scan's item count is an int
    const int64_t n = ta.count;
    if (n == 0) {
        for (int c = 0; c < ta.n_cols; ++c)
            if (ta.cols[c].kind == 1 && hipMemsetAsync(ta.cols[c].i64, 0, 8, s) != hipSuccess) return -1;
        return 0;
    }
    if (table_ext(ta)) {
        if (hipMemsetAsync(ta.bad_row, 0, 4, s) != hipSuccess) return -1;
        if (has_geo(ta)) hipLaunchKernelGGL((k_table_values<true, true>), dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, s, d_args, d_targs, buf);
        else hipLaunchKernelGGL((k_table_values<true, false>), dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, s, d_args, d_targs, buf);
    } else {
        if (has_geo(ta)) hipLaunchKernelGGL((k_table_values<false, true>), dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, s, d_args, d_targs, buf);
        else hipLaunchKernelGGL((k_table_values<false, false>), dim3((unsigned)((n + TB - 1) / TB)), dim3(TB), 0, s, d_args, d_targs, buf);
    }
    if (mid) hipEventRecord(mid, s);  // the values kernel done: the scans follow
    if (!offsets) return hipGetLastError() == hipSuccess ? 0 : -1;  // i64[k + 1] stays row k's length (dict.hip)
    size_t tmp = 0;
    hipcub::DeviceScan::InclusiveSum(nullptr, tmp, (const int64_t*)nullptr, (int64_t*)nullptr, (int)n);
    const size_t tmp_al = (tmp + 255) & ~(size_t)255;
    if (tmp_al + 8 * (size_t)n > scratch_bytes) return -1;
    int64_t* sums = reinterpret_cast<int64_t*>((char*)scratch + tmp_al);
    for (int c = 0; c < ta.n_cols; ++c) {
        if (ta.cols[c].kind != 1) continue;
        int64_t* off = (int64_t*)ta.cols[c].i64;
        size_t t = tmp;
        if (hipcub::DeviceScan::InclusiveSum(scratch, t, off + 1, sums, (int)n, s) != hipSuccess) return -1;
        if (hipMemcpyAsync(off + 1, sums, 8 * (size_t)n, hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_table_chars(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const uint8_t* buf,
                       hipStream_t s) {
    int n_str = 0;
    for (int c = 0; c < ta.n_cols; ++c) n_str += ta.cols[c].kind == 1 ? 1 : 0;
    if (ta.count == 0 || n_str == 0) return 0;
    const int64_t waves = (ta.count + 63) / 64;
    const dim3 grid((unsigned)((waves + CW - 1) / CW), (unsigned)n_str);
    if (ta.rows) hipLaunchKernelGGL(k_table_chars<true>, grid, dim3(64 * CW), 0, s, d_args, d_targs, buf);
    else hipLaunchKernelGGL(k_table_chars<false>, grid, dim3(64 * CW), 0, s, d_args, d_targs, buf);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- map columns: the scratch of one column (lp_table.h MapArgs).  The per-row
// arrays come first: their place depends on count alone, so they survive a
// second layout with the piece count known.
namespace {
struct MapLayout {
    size_t cnt, pbase, bad_row, tmp, tmp_bytes, flag, eidx, klen, vlen, kpos, vpos, ksrc, vsrc, total;
};
MapLayout map_layout(int64_t count, int64_t pieces) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    MapLayout L{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += al(bytes); return o; };
    const size_t rows = (size_t)count + 1, pcs = (size_t)pieces + 1;
    L.cnt = take(8 * rows);
    L.pbase = take(8 * rows);
    L.bad_row = take(4);
    size_t t1 = 0, t2 = 0, t3 = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, t1, (const int64_t*)nullptr, (int64_t*)nullptr, (int)rows);
    hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)pcs);
    hipcub::DeviceScan::ExclusiveSum(nullptr, t3, (const int64_t*)nullptr, (int64_t*)nullptr, (int)pcs);
    L.tmp_bytes = t1 > t2 ? t1 : t2;
    L.tmp_bytes = L.tmp_bytes > t3 ? L.tmp_bytes : t3;
    L.tmp = take(L.tmp_bytes);
    L.flag = take(4 * pcs);
    L.eidx = take(4 * pcs);
    L.klen = take(8 * pcs);
    L.vlen = take(8 * pcs);
    L.kpos = take(8 * pcs);
    L.vpos = take(8 * pcs);
    L.ksrc = take(8 * pcs);
    L.vsrc = take(8 * pcs);
    L.total = at;
    return L;
}
MapLayout map_bind(MapArgs& ma, void* scratch) {
    const MapLayout L = map_layout(ma.count, ma.n_pieces);
    char* b = (char*)scratch;
    // (a C-style cast: in the device pass the members are global-memory pointers)
    auto at = [&](auto& dst, size_t off) { dst = (std::remove_reference_t<decltype(dst)>)(b + off); };
    at(ma.cnt, L.cnt);
    at(ma.pbase, L.pbase);
    at(ma.bad_row, L.bad_row);
    at(ma.flag, L.flag);
    at(ma.eidx, L.eidx);
    at(ma.klen, L.klen);
    at(ma.vlen, L.vlen);
    at(ma.kpos, L.kpos);
    at(ma.vpos, L.vpos);
    at(ma.ksrc, L.ksrc);
    at(ma.vsrc, L.vsrc);
    at(ma.ksrc_e, L.klen);
    at(ma.vsrc_e, L.vlen);
    return L;
}
unsigned blocks_of(int64_t n) { return (unsigned)((n + TB - 1) / TB); }
}  // namespace

size_t map_scratch_bytes(int64_t count, int64_t pieces) { return map_layout(count, pieces).total; }

int launch_map_count(const DeviceArgs* d_args, MapArgs& ma, void* scratch, size_t scratch_bytes, hipStream_t s,
                     const int64_t** total) {
    if (ma.count < 0 || ma.count >= 0x7FFFFFFF) return -1;  // the scan's item count is an int
    ma.n_pieces = 0;
    const MapLayout L = map_bind(ma, scratch);
    if (L.total > scratch_bytes) return -1;
    const int rows = (int)ma.count + 1;
    if (ma.rows) {
        if (hipMemsetAsync(ma.bad_row, 0, 4, s) != hipSuccess) return -1;
        hipLaunchKernelGGL(k_map_count<true>, dim3(blocks_of(rows)), dim3(TB), 0, s, d_args, ma);
    } else {
        hipLaunchKernelGGL(k_map_count<false>, dim3(blocks_of(rows)), dim3(TB), 0, s, d_args, ma);
    }
    size_t t = L.tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum((char*)scratch + L.tmp, t, (const int64_t*)ma.cnt, (int64_t*)ma.pbase, rows, s) !=
        hipSuccess)
        return -1;
    *total = (const int64_t*)ma.pbase + ma.count;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_map_entries(const DeviceArgs* d_args, MapArgs& ma, const uint8_t* buf, void* scratch, size_t scratch_bytes,
                       hipStream_t s, const void* totals[3]) {
    if (ma.n_pieces <= 0 || ma.n_pieces >= 0x7FFFFFFF) return -1;
    const MapLayout L = map_bind(ma, scratch);
    if (L.total > scratch_bytes) return -1;
    const int pcs = (int)ma.n_pieces + 1;
    if (ma.rows) hipLaunchKernelGGL(k_map_entries<true>, dim3(blocks_of(pcs)), dim3(TB), 0, s, d_args, ma, buf);
    else hipLaunchKernelGGL(k_map_entries<false>, dim3(blocks_of(pcs)), dim3(TB), 0, s, d_args, ma, buf);
    void* tmp = (char*)scratch + L.tmp;
    size_t t = L.tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(tmp, t, (const uint32_t*)ma.flag, (uint32_t*)ma.eidx, pcs, s) != hipSuccess) return -1;
    t = L.tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(tmp, t, (const int64_t*)ma.klen, (int64_t*)ma.kpos, pcs, s) != hipSuccess) return -1;
    t = L.tmp_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(tmp, t, (const int64_t*)ma.vlen, (int64_t*)ma.vpos, pcs, s) != hipSuccess) return -1;
    totals[0] = (const uint32_t*)ma.eidx + ma.n_pieces;
    totals[1] = (const int64_t*)ma.kpos + ma.n_pieces;
    totals[2] = (const int64_t*)ma.vpos + ma.n_pieces;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_map_fill(MapArgs& ma, int64_t n_entries, void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (ma.n_pieces <= 0 || n_entries < 0 || n_entries > ma.n_pieces) return -1;
    const MapLayout L = map_bind(ma, scratch);
    if (L.total > scratch_bytes) return -1;
    const int64_t n = (ma.n_pieces > ma.count ? ma.n_pieces : ma.count) + 1;
    hipLaunchKernelGGL(k_map_fill, dim3(blocks_of(n)), dim3(TB), 0, s, ma);
    if (n_entries > 0) {
        const int64_t waves = (n_entries + 63) / 64;
        hipLaunchKernelGGL(k_map_chars, dim3((unsigned)((waves + CW - 1) / CW), 2u), dim3(64 * CW), 0, s, ma, n_entries);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lp
