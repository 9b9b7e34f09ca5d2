// The GeoIP value stages on the device (lp_program.h ValStage, VK_GEOIP;
// lp_geoip.h): k_geoip_lines, one line per lane, after the parse and URI
// kernels.  For each GeoIP stage of the line's LogFormat it takes the IP
// token's span, stages the token's bytes (at most 45) in registers with
// aligned 16-byte loads, parses the address text (ip_parse_words) and walks
// the stage's tree image with one 8-byte load per level (geo_walk): lanes are
// independent, a lane leaves the loop at its leaf, and the upper levels of
// the tree are shared by every lane, so they stay in cache.  It writes
// geo[stage][line] = record id + 1 (0: null / empty token, or not in the tree)
// and sends a line whose text is outside the decided subset to FALLBACK,
// moving it between the batch's counters as k_derived_lines does.
// No shortcut over the first address bits: the plain walk.
#include "kernels_common.h"
#include "lp_geoip.h"

namespace lp {

namespace {

__global__ __launch_bounds__(PW) void k_geoip_lines(const uint8_t* __restrict__ buf, uint64_t nbytes,
                                                    const DeviceArgs* __restrict__ args) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const int64_t n_lines = (int64_t)C.meta->n_lines;
    const int64_t li0 = (int64_t)blockIdx.x * PW;
    if (li0 >= n_lines || C.meta->cap_ovf) return;
    const int64_t li = li0 + lane_id();
    const bool active = li < n_lines;
    int st = active ? (int)C.status[li] : -1;
    const bool was_ok = st == ST_OK;
    const int fmt = was_ok && P.n_fmt > 1 ? (int)C.fmt_id[li] : 0;
    const uint64_t ls = active ? C.line_off[li] : 0;
    const uint32_t flags = was_ok ? C.tok_flags[li] : 0u;
    for (int k = 0; k < P.n_val; ++k) {
        const ValStage& S = P.val[k];
        if (S.kind != VK_GEOIP) continue;  // (uniform: the program)
        uint32_t rec = 0;
        if (was_ok && S.fmt == fmt && !((flags >> S.src_tok) & 1u)) {
            const uint32_t sp = C.tok_span[S.src_tok][li];
            const uint32_t off = sp & 0xFFFFu, n = (sp >> 16) - off;
            // (inside the line: line_off[li] + off + n <= line_off[li + 1] <= nbytes + 1)
            if (n > 0 && ls + off + n <= nbytes) {
                int fam = IPF_UNDECIDED;
                uint32_t a[4] = {0, 0, 0, 0};
                if (n <= (uint32_t)GEO_MAX_TEXT) {
                    // the token's bytes from the aligned 16-byte blocks that hold them (each holds a
                    // byte of the input, so it lies inside the input's allocation granule), moved to
                    // byte 0 of w (ip_align_words)
                    const LP_G uint8_t* tp = (const LP_G uint8_t*)buf + ls + off;
                    const uint32_t m = (uint32_t)((uintptr_t)tp & 15u);
                    const LP_G uint4* blk = reinterpret_cast<const LP_G uint4*>(tp - m);
                    uint32_t x[16];
                    LP_UNROLL
                    for (int j = 0; j < 4; ++j) {
                        uint4 v = make_uint4(0, 0, 0, 0);
                        if (16u * (uint32_t)j < m + n) v = blk[j];
                        x[4 * j] = v.x;
                        x[4 * j + 1] = v.y;
                        x[4 * j + 2] = v.z;
                        x[4 * j + 3] = v.w;
                    }
                    uint32_t w[12];
                    ip_align_words(x, m, w);
                    fam = ip_parse_words(w, n, a);
                }
                const LP_G uint64_t* img = C.geo_tree[k];
                const int64_t r = geo_resolve(img, a, fam);
                if (r < 0) st = ST_FALLBACK;  // the reference owns the line
                else rec = (uint32_t)r;
            }
        }
        if (active) C.geo[k][li] = rec;
    }
    if (was_ok && st != ST_OK) C.status[li] = (uint8_t)st;
    // the batch's counters are sums that the reduction after this kernel adds to: move the lines
    // taken from OK to FALLBACK (the sums commute)
    const unsigned long long fb = __popcll(__ballot(was_ok && st == ST_FALLBACK));
    if (lane_id() == 0 && fb) {
        atomicAdd(&C.meta->counters[1], 0ull - fb);
        atomicAdd(&C.meta->counters[3], fb);
    }
}

}  // namespace

int launch_geoip(const ParseLaunch& a, const DeviceArgs* d_args, hipStream_t s) {
    const int64_t waves = parse_waves(a.cap_lines);
    if (waves == 0 || !a.geoip) return 0;
    if (a.geo_event[0]) (void)hipEventRecord((hipEvent_t)a.geo_event[0], s);
    hipLaunchKernelGGL(k_geoip_lines, dim3((unsigned)waves), dim3(PW), 0, s, a.buf, a.nbytes, d_args);
    if (a.geo_event[1]) (void)hipEventRecord((hipEvent_t)a.geo_event[1], s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lp
