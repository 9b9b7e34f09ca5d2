// TEST-ONLY: the CPU emulation of tests/emu/emu.cpp with the parser's added
// dissectors (Parser.addDissector: Plan::build's dissectors argument).  The
// shared machinery is emu.cpp's own, included as it is; this unit only adds
// the compile entry and the possible-paths entry that take dissectors.
#include "emu.cpp"

// k_derived_lines of a program without URI, list or pair stages: emu.cpp's
// run_line stops after phase 1 there (nothing else ran before the value
// stages), the kernels still launch k_derived_lines for the guard of a token's
// value stage (uri.hip launch_uri).  Phase 1 again on the line, as
// k_parse_ovf_lines parses it (HBM bytes), then derived_line on the columns it
// wrote.  Returns the line's status.
static int token_guard(Emu* e, const char* line, int len) {
    const Program& P = e->plan.program();
    bool any = false;
    for (int k = 0; k < P.n_val; ++k) any = any || (P.val[k].kind == VK_SCREEN && P.val[k].src_tok >= 0);
    if (P.has_phase2() || !any) return ST_OK;
    std::vector<uint32_t> padded(((size_t)len + 16) / 4 + 4, 0xFFFFFFFFu);  // (4-byte aligned, word reads past the end)
    uint8_t* base = (uint8_t*)padded.data();
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
    Arena D{nullptr, 0, 0};
    return derived_line(P, o.fmt, base, 0u, len, D, C, 0);
}

extern "C" {

// emu_parse / emu_parse_in, then the value stages' guard where emu.cpp's run_line does not reach it
int emu_parse_guarded(void* h, const char* line, int len, char* out, int cap) {
    const int st = emu_parse(h, line, len, out, cap);
    return st == 0 ? token_guard((Emu*)h, line, len) : st;
}
int emu_parse_in_guarded(void* h, const char* buf, int64_t start, int len, char* out, int cap) {
    const int st = emu_parse_in(h, buf, start, len, out, cap);
    return st == 0 ? token_guard((Emu*)h, buf + start, len) : st;
}


// emu_new_remapped with added dissectors ds_name[k] / ds_settings[k].
// *status: the planner's (0 OK, -3 unsupported: both give a handle; -1 invalid,
// -2 missing: null, err filled)
void* emu_new_dissectors(const char* fmt, const char* const* fields, int n, const char* const* rm_in,
                         const char* const* rm_type, int n_rm, const char* const* ds_name,
                         const char* const* ds_settings, int n_ds, int* status, char* err, int errlen) {
    Emu* e = new Emu();
    std::vector<std::string> f(fields, fields + n);
    std::vector<Remap> rm;
    for (int k = 0; k < n_rm; ++k) rm.push_back(Remap{rm_in[k], rm_type[k], CAST_S});
    std::vector<AddDissector> ds;
    for (int k = 0; k < n_ds; ++k) ds.push_back(AddDissector{ds_name[k], ds_settings[k]});
    e->status = e->plan.build(fmt, f, e->err, rm, ds);
    *status = e->status;
    if (err && errlen) snprintf(err, errlen, "%s%s", e->err.c_str(), e->plan.device_ok() ? "" : e->plan.unsupported_reason().c_str());
    if (e->status != 0 && e->status != -3) { delete e; return nullptr; }
    return e;
}

// Parser.getPossiblePaths with type remappings and added dissectors; the
// planner's status when it refuses (an unknown class), else the text's length
int emu_possible_paths_dissectors(const char* fmt, int depth, const char* const* rm_in, const char* const* rm_type,
                                  int n_rm, const char* const* ds_name, const char* const* ds_settings, int n_ds,
                                  char* out, int cap) {
    std::vector<Remap> rm;
    for (int k = 0; k < n_rm; ++k) rm.push_back(Remap{rm_in[k], rm_type[k], CAST_S});
    std::vector<AddDissector> ds;
    for (int k = 0; k < n_ds; ++k) ds.push_back(AddDissector{ds_name[k], ds_settings[k]});
    std::vector<std::string> paths;
    std::string err;
    const int st = Plan::possible_paths(fmt, depth, paths, err, rm, ds);
    if (st != 0) return st;
    std::string s;
    for (auto& p : paths) s += p + "\n";
    if ((int)s.size() + 1 > cap) return -100;
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}
}
