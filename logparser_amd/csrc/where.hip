// gfx950 kernel of lp_result_select_where on a device view (include/
// logparser_amd.h): the lines of a window whose status is in a mask and on
// whose table row a predicate holds, as one bit per line --
//
//   k_where_eval    one lane per line: the status test, then term by term the
//                   value lp_result_table_rows would build for the line and
//                   the term's (path, kind) column -- derived by tvalue_any
//                   from the parse kernels' SoA columns, never written to a
//                   column -- the term's rule (lp_pred.h) and the fold; a
//                   __ballot word per wave
//
// select.hip's two passes then take their 16-bit match words from those bits
// instead of the status bytes: the predicate is evaluated once.
//
// The "value of (column, row)" step restates k_table_values' (table.hip): the
// pseudo-columns before the status test, then the later delivery (src), then
// -- a value that is none for the column -- the earlier (alt).  It is a
// second copy on purpose: k_table_values' instances keep the code and the
// registers they had.
#include <hip/hip_runtime.h>

#define LP_KERNEL_TU 1  // device column pointers are global-memory pointers (lp_program.h)

#include "kernels_common.h"  // lane_id
#include "lp_pred.h"
#include "table_value.h"  // TVal, tvalue_any, has_geo

namespace lp {

namespace {

constexpr int WB = 256;  // lines per block: four waves, each 64 consecutive lines and one word of bits

template <bool EXT, bool GEO>
__global__ __launch_bounds__(WB) void k_where_eval(const DeviceArgs* __restrict__ args, const TableArgs* __restrict__ targs,
                                                   const uint8_t* buf, const WhereArgs W) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const TableArgs& T = *targs;
    const int64_t j = (int64_t)blockIdx.x * WB + threadIdx.x;  // the line, counted from the first 16-line group
    const int64_t i = (W.first & ~(int64_t)15) + j;
    // 1. the status, before any value is derived (a lane outside the window: no line)
    bool in = i >= W.first && i < W.first + W.count;
    uint32_t st = ST_BAD;
    if (in) {
        st = C.status[i];
        in = ((W.mask >> (st & 7u)) & 1u) != 0;
    }
    const bool ok = in && st == ST_OK;
    const LP_G uint8_t *line = nullptr, *region = nullptr;
    if (ok) {  // (row_view, the status known)
        line = (const LP_G uint8_t*)buf + C.line_off[i];
        region = P.has_phase2() ? C.arena + C.arena_base[i] : C.arena;
    }
    const int fmt = ok && P.n_fmt > 1 ? (int)C.fmt_id[i] : 0;
    PredFold F;
    F.live = in;
    for (int t = 0; t < W.n_terms; ++t) {
        const WhereTerm& R = W.t[t];  // (the same term in every lane: wave-uniform reads)
        pred_fold_group(F, t, R.group);
        // a line decided false derives no further value; a wave without a live lane skips the rest
        if (__ballot(F.live) == 0) break;
        if (!pred_fold_wants(F)) continue;
        const TableCol& col = T.cols[t];
        TVal v;
        bool valid = false;
        if constexpr (EXT) {
            // 2. a pseudo-column: valid for every status
            const int32_t pk = col.src[0].kind;
            if (tc_pseudo(pk)) {
                valid = true;
                if (pk == TC_LINE) {  // the parse kernels' line: wave_lines' end, crlf_len
                    const uint64_t s0 = C.line_off[i], e0 = C.line_off[i + 1] - 1;
                    const LP_G uint8_t* lp = (const LP_G uint8_t*)buf + s0;
                    uint64_t n = e0 - s0;
                    if (n > 0 && lp[n - 1] == '\r') --n;
                    v.kind = 1;
                    v.p = lp;
                    v.n = (uint32_t)n;
                } else {
                    v.kind = 2;
                    v.l = pk == TC_OFFSET ? (int64_t)C.line_off[i] : pk == TC_LINENO ? T.first_line + i : (int64_t)st;
                }
            }
        }
        // 3. the later delivery, then (a value that is none for the column) the earlier
        for (int pass = 0; pass < 2 && ok && !valid; ++pass) {
            const TableSrc& sc = pass ? col.alt[fmt] : col.src[fmt];
            if (pass && sc.kind == TC_NONE) break;
            v = tvalue_any<GEO>(P, C, T, sc, i, line, region);
            valid = v.kind != 0;
            if (col.kind == 2) {  // LONG: parse_long of text; month names, dates: not numbers
                if (v.kind == 1) {
                    int64_t x = 0;
                    valid = parse_long(v.p, v.n, v.amp, x);
                    v.kind = 2;
                    v.l = x;
                } else if (v.kind == 3) {
                    valid = false;
                }
            }
        }
        // 4. the term's rule
        bool r;
        if (col.kind == 2) {
            r = pred_term_long(R.op, !valid, v.l, R.lo, R.hi);
        } else {
            const uint8_t* o = T.names + R.str_off;
            if (valid && v.kind == 2) {  // a STRING taken from a long: its decimal text
                v.n = digits(v.l);
                write_long(v.buf, v.l, v.n);
                v.kind = 3;
            }
            if (valid && v.kind == 1) {
                PredWords<const LP_G uint8_t*, const LP_G uint32_t*> view{v.p, v.n, v.amp};
                r = pred_term_bytes(R.op, false, view, o, (uint32_t)R.str_len);
            } else {
                PredLocal view{v.buf, valid ? v.n : 0u};
                r = pred_term_bytes(R.op, !valid, view, o, (uint32_t)R.str_len);
            }
        }
        pred_fold_term(F, r);
    }
    // 5. the fold; the wave's 64 lines are one word of the bits
    const bool sel = in && pred_fold_result(F, W.n_terms);
    const uint64_t word = __ballot(sel);
    // (the block's last waves may lie wholly past the window: they have no word)
    if (lane_id() == 0 && j < (W.first & 15) + W.count) W.bits[j >> 6] = word;
}

}  // namespace

int launch_where_eval(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const uint8_t* buf,
                      const WhereArgs& wa, hipStream_t s) {
    if (wa.first < 0 || wa.count <= 0 || !wa.bits || wa.n_terms < 0 || wa.n_terms > WHERE_MAX_TERMS) return -1;
    const int64_t span = (wa.first & 15) + wa.count;
    const int64_t blocks = (span + WB - 1) / WB;
    if (blocks >= 0x7FFFFFFF) return -1;
    const dim3 grid((unsigned)blocks), tb(WB);
    bool ext = false;  // a pseudo-column term (the same for every LogFormat)
    for (int c = 0; c < ta.n_cols; ++c) ext = ext || tc_pseudo(ta.cols[c].src[0].kind);
    const bool geo = has_geo(ta);
    if (ext && geo) hipLaunchKernelGGL((k_where_eval<true, true>), grid, tb, 0, s, d_args, d_targs, buf, wa);
    else if (ext) hipLaunchKernelGGL((k_where_eval<true, false>), grid, tb, 0, s, d_args, d_targs, buf, wa);
    else if (geo) hipLaunchKernelGGL((k_where_eval<false, true>), grid, tb, 0, s, d_args, d_targs, buf, wa);
    else hipLaunchKernelGGL((k_where_eval<false, false>), grid, tb, 0, s, d_args, d_targs, buf, wa);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lp
