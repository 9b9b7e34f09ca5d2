// TEST-ONLY: the CPU emulation (tests/emu/emu.cpp with dissectors_emu.cpp's
// entry points for added dissectors) plus k_geoip_lines' per-line work
// (logparser_amd/csrc/geoip.hip): phase 1 again on the line, as
// dissectors_emu.cpp's token_guard, then for every GeoIP stage of the line's
// format the token staged as the kernel stages it -- the aligned 16-byte
// blocks that hold it, ip_align_words -- ip_parse_words and geo_resolve of
// logparser_amd/csrc/lp_geoip.h on the plan's tree image.  The record's
// values come from the replay (Plan::run_phase), which looks the value up
// with the same functions when a view has no geo column.
#include "dissectors_emu.cpp"

#include "../../logparser_amd/csrc/lp_geoip.h"

// the line's status after k_geoip_lines, rec[k] = column geo of value stage k
static int geo_lines(Emu* e, const char* line, int len, uint32_t* rec) {
    const Program& P = e->plan.program();
    for (int k = 0; k < MAX_VAL; ++k) rec[k] = 0;
    bool any = false;
    for (int k = 0; k < P.n_val; ++k) any = any || P.val[k].kind == VK_GEOIP;
    if (!any) return ST_OK;
    // (16-byte aligned, as the device's input; the blocks around the line are readable)
    std::vector<uint32_t> padded(((size_t)len + 96) / 4 + 8, 0x2E2E2E2Eu);
    uint8_t* base = (uint8_t*)(((uintptr_t)padded.data() + 15) & ~(uintptr_t)15);
    memcpy(base, line, (size_t)len);
    base[len] = '\n';
    std::vector<uint8_t> status(1);
    std::vector<uint32_t> tok_flags(1);
    std::vector<std::vector<uint32_t>> u32(MAX_TOK + 4 * MAX_FL + MAX_TIME + MAX_BINIP, std::vector<uint32_t>(1));
    std::vector<std::vector<uint64_t>> u64(3 * MAX_TIME + MAX_SECMS, std::vector<uint64_t>(1));
    Columns C;
    memset(&C, 0, sizeof C);
    C.status = status.data();
    C.tok_flags = tok_flags.data();
    int a = 0, b = 0;
    for (int k = 0; k < MAX_TOK; ++k) C.tok_span[k] = u32[a++].data();
    for (int f = 0; f < MAX_FL; ++f) {
        C.fl_kind[f] = u32[a++].data(); C.fl_method[f] = u32[a++].data();
        C.fl_uri[f] = u32[a++].data(); C.fl_proto[f] = u32[a++].data();
    }
    for (int t = 0; t < MAX_TIME; ++t) {
        C.t_nano[t] = u32[a++].data();
        C.t_epoch[t] = (int64_t*)u64[b++].data(); C.t_local[t] = u64[b++].data(); C.t_utc[t] = u64[b++].data();
    }
    for (int k = 0; k < MAX_BINIP; ++k) C.bip[k] = u32[a++].data();
    for (int k = 0; k < MAX_SECMS; ++k) C.sm_ms[k] = (int64_t*)u64[b++].data();
    LineOut o;
    uint32_t stk[MAX_STACK];
    const Line L{base, 0u, len};
    const int fmt = P.n_fmt > 1 ? (int)e->fmt_state : 0;  // (the state emu_parse left: the line's routed format)
    if (P.n_fmt > 1) phase1<false>(P, P.elems, L, o, stk, C, 0, false, fmt);
    else if (lit_aware(P)) phase1<false, true>(P, P.elems, L, o, stk, C, 0, false, 0);
    else phase1<false, false>(P, P.elems, L, o, stk, C, 0, false, 0);
    write_line(P, o, C, 0);
    if (o.status != ST_OK) return o.status;
    int st = ST_OK;
    for (int k = 0; k < P.n_val; ++k) {
        const ValStage& S = P.val[k];
        if (S.kind != VK_GEOIP || S.fmt != o.fmt || ((C.tok_flags[0] >> S.src_tok) & 1u)) continue;
        const uint32_t sp = C.tok_span[S.src_tok][0];
        const uint32_t off = sp & 0xFFFFu, n = (sp >> 16) - off;
        if (n == 0) continue;
        int fam = IPF_UNDECIDED;
        uint32_t ad[4] = {0, 0, 0, 0};
        if (n <= (uint32_t)GEO_MAX_TEXT) {
            const uint8_t* tp = base + off;
            const uint32_t m = (uint32_t)((uintptr_t)tp & 15u);
            uint32_t x[16];
            for (int j = 0; j < 4; ++j) {
                if (16u * (uint32_t)j < m + n) memcpy(x + 4 * j, tp - m + 16 * j, 16);
                else memset(x + 4 * j, 0, 16);
            }
            uint32_t w[12];
            ip_align_words(x, m, w);
            fam = ip_parse_words(w, n, ad);
        }
        const int64_t r = geo_resolve(e->plan.geo_image(k).tree->data(), ad, fam);
        if (r < 0) st = ST_FALLBACK;
        else rec[k] = (uint32_t)r;
    }
    return st;
}

extern "C" {

// emu_parse_guarded / emu_parse_in_guarded, then k_geoip_lines; rec: MAX_VAL words
int emu_parse_geo(void* h, const char* line, int len, char* out, int cap, uint32_t* rec) {
    const int st = emu_parse_guarded(h, line, len, out, cap);
    return st == 0 ? geo_lines((Emu*)h, line, len, rec) : st;
}
int emu_parse_in_geo(void* h, const char* buf, int64_t start, int len, char* out, int cap, uint32_t* rec) {
    const int st = emu_parse_in_guarded(h, buf, start, len, out, cap);
    return st == 0 ? geo_lines((Emu*)h, buf + start, len, rec) : st;
}
}
