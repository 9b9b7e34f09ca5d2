// TEST-ONLY CPU unit for the straight-line first leaf of the fixed-shape
// instances (logparser_amd/csrc/lp_device.h fixed_fast_leaf), built to a
// library of its own (tests/fixed_fast_emu_lib.py) and, with -DFF_MAIN, to a
// stand-alone program that runs a corpus file under the sanitizers.
//
// Every line is laid at a chosen offset of a 64-byte aligned window with
// mask planes and goes through
//   fixed_fast_leaf<SHAPE>      it may only accept: when it does, the generic
//                               match_first_leaf<false, true> must succeed
//                               with the same spans, and nothing is written
//                               when it declines
//   match_fixed_leaf<SHAPE>     (fast leaf, else the element walk) against
//                               match_first_leaf<false, true>: boolean, spans
//   phase1<..., SHAPE>          against the SIMPLE phase 1: the whole LineOut
// and the lines the fast leaf accepted / left to the walk are counted.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../logparser_amd/csrc/lp_device.h"
#include "../../logparser_amd/csrc/plan.h"

using namespace lp;

namespace {

struct Ff {
    Plan plan;
    std::string err;
    int shape = FS_NONE;
};

bool same_out(const LineOut& x, const LineOut& y, std::string* why) {
    auto arr = [&](const char* name, const uint32_t* p, const uint32_t* q, int n) {
        for (int k = 0; k < n; ++k)
            if (p[k] != q[k]) {
                *why = std::string("phase 1: ") + name + "[" + std::to_string(k) + "]";
                return false;
            }
        return true;
    };
    if (x.status != y.status) {
        *why = "phase 1: status " + std::to_string(x.status) + " / " + std::to_string(y.status);
        return false;
    }
    if (x.status != ST_OK) return true;  // (a line that is not OK delivers nothing else)
    if (x.tok_flags != y.tok_flags || x.tdone != y.tdone || x.hist != y.hist) {
        *why = "phase 1: tok_flags / tdone / hist";
        return false;
    }
    return arr("caps", x.caps.v, y.caps.v, MAX_TOK) && arr("fl_kind", x.fl_kind.v, y.fl_kind.v, MAX_FL) &&
           arr("fl_method", x.fl_method.v, y.fl_method.v, MAX_FL) && arr("fl_uri", x.fl_uri.v, y.fl_uri.v, MAX_FL) &&
           arr("fl_proto", x.fl_proto.v, y.fl_proto.v, MAX_FL) && arr("ep_lo", x.ep_lo.v, y.ep_lo.v, MAX_TIME) &&
           arr("ep_hi", x.ep_hi.v, y.ep_hi.v, MAX_TIME) && arr("lo_lo", x.lo_lo.v, y.lo_lo.v, MAX_TIME) &&
           arr("lo_hi", x.lo_hi.v, y.lo_hi.v, MAX_TIME) && arr("ut_lo", x.ut_lo.v, y.ut_lo.v, MAX_TIME) &&
           arr("ut_hi", x.ut_hi.v, y.ut_hi.v, MAX_TIME) && arr("nano", x.nano.v, y.nano.v, MAX_TIME);
}

// what one line view did: bit 0 the fast leaf accepted, bit 1 the chunk
// kernel would count it in walk_lines (phase 1 reached the match and took the
// element walk); status: the SIMPLE phase 1's
struct Seen {
    int fast = 0, walked = 0, status = 0;
};

// One line at byte off (0..63) of a 64-byte aligned window whose other bytes
// are quotes, spaces and a terminator, as neighbouring lines would leave
// them (so the plane bits next to the line are set).  The planes hold exactly
// the window's blocks: a read of any other block is out of bounds (ASan).
template <int SHAPE>
bool check_line(const Program& P, const uint8_t* line, int n, int off, Seen* seen, std::string* why) {
    const uint32_t wn = (uint32_t)((off + n + 1 + 63) & ~63);
    std::vector<uint8_t> wv(wn + 8);
    uint8_t* w = wv.data();
    static const char fill[] = "\" \"x ";
    for (uint32_t k = 0; k < wn + 8; ++k) w[k] = (uint8_t)fill[k % 5];
    if (off) w[off - 1] = '\n';
    memcpy(w + off, line, (size_t)n);
    w[off + n] = '\n';
    std::vector<uint64_t> masks(MC_N * (wn / 64));
    build_masks(w, wn, masks.data());
    const MLine M{w, (uint32_t)off, n, masks.data()};
    // the fast leaf alone
    RegArr<MAX_TOK> g, f, m;
    g.fill(0);
    f.fill(0x5A5A5A5Au);
    m.fill(0);
    const bool rg = match_first_leaf<false, true>(P, M, g);
    const bool rf = fixed_fast_leaf<SHAPE>(M, f);
    seen->fast = rf ? 1 : 0;
    if (rf) {
        if (!rg) { *why = "the fast leaf accepted a line the generic first leaf does not match"; return false; }
        for (int k = 0; k < fixed_shape(SHAPE).n_tok; ++k)
            if (f.v[k] != g.v[k]) { *why = "fast leaf: span " + std::to_string(k); return false; }
        for (int k = fixed_shape(SHAPE).n_tok; k < MAX_TOK; ++k)
            if (f.v[k] != 0x5A5A5A5Au) { *why = "fast leaf wrote slot " + std::to_string(k); return false; }
    } else {
        for (int k = 0; k < MAX_TOK; ++k)
            if (f.v[k] != 0x5A5A5A5Au) { *why = "the fast leaf declined but wrote slot " + std::to_string(k); return false; }
    }
    // the instance's first leaf (fast, else the walk)
    bool walked = false;
    const bool rm = match_fixed_leaf<SHAPE, false>(P, M, m, &walked);
    if (rm != rg || walked == rf) { *why = "match_fixed_leaf: result / path"; return false; }
    for (int k = 0; k < MAX_TOK; ++k)
        if (m.v[k] != g.v[k]) { *why = "match_fixed_leaf: span " + std::to_string(k); return false; }
    // the whole phase 1 (the chunk kernel's: no DFS)
    Columns C;
    memset(&C, 0, sizeof C);
    uint32_t stk[MAX_STACK];
    LineOut x, y;
    memset(&x, 0, sizeof x);
    memset(&y, 0, sizeof y);
    phase1<false, false, true, false>(P, P.elems, M, x, stk, C, 0, false, 0);
    phase1<false, false, true, false, false, SHAPE>(P, P.elems, M, y, stk, C, 0, false, 0);
    seen->status = x.status;
    seen->walked = (int)y.walked;
    if (x.walked != 0) { *why = "the SIMPLE instance set walked"; return false; }
    return same_out(x, y, why);
}

bool check_line_shape(int shape, const Program& P, const uint8_t* line, int n, int off, Seen* seen, std::string* why) {
    switch (shape) {
    case FS_COMBINED: return check_line<FS_COMBINED>(P, line, n, off, seen, why);
    case FS_COMMON: return check_line<FS_COMMON>(P, line, n, off, seen, why);
    }
    *why = "no such shape";
    return false;
}

// Every '\n'-terminated line of buf[0, n) at window offset off (0..63), at
// every offset (off == -2) or line i at offset i mod 64 (off == -1).  stats:
// [0] line views, [1] fast-leaf accepts, [2] walk_lines (as the kernel counts
// them), [3] OK, [4] BAD, [5] FALLBACK, [6] REDO, [7] lines whose accept
// differs between two offsets.  flags (optional): per line, bit 0 the fast
// leaf accepted, bit 1 counted in walk_lines (at the last offset tried).
int64_t run(const Ff& f, const uint8_t* buf, int64_t n, int off, int64_t* stats, uint8_t* flags, std::string* first) {
    const Program& P = f.plan.program();
    int64_t bad = 0, i = 0;
    for (int k = 0; k < 8; ++k) stats[k] = 0;
    for (int64_t s = 0; s < n; ++i) {
        const uint8_t* nl = (const uint8_t*)memchr(buf + s, '\n', (size_t)(n - s));
        const int64_t e = nl ? nl - buf : n;
        const int o0 = off == -2 ? 0 : off == -1 ? (int)(i & 63) : off, o1 = off == -2 ? 64 : o0 + 1;
        int fast0 = -1;
        Seen seen;
        for (int o = o0; o < o1; ++o) {
            std::string why;
            seen = Seen{};
            if (!check_line_shape(f.shape, P, buf + s, (int)(e - s), o, &seen, &why)) {
                if (!bad++ && first) *first = "line " + std::to_string(i) + " at offset " + std::to_string(o) + ": " + why;
            }
            ++stats[0];
            stats[1] += seen.fast;
            stats[2] += seen.walked;
            if (seen.status >= 0 && seen.status <= 3) ++stats[3 + seen.status];
            if (fast0 >= 0 && fast0 != seen.fast) ++stats[7];
            fast0 = seen.fast;
        }
        if (flags) flags[i] = (uint8_t)(seen.fast | (seen.walked << 1));
        s = e + 1;
    }
    return bad;
}

int build(Ff& f, const char* name) {
    std::vector<std::string> paths;
    if (Plan::possible_paths(name, 15, paths, f.err) != 0 || f.plan.build(name, paths, f.err) != 0) return 2;
    f.shape = f.plan.device_ok() ? fixed_shape_of(f.plan.program()) : FS_NONE;
    return f.shape == FS_NONE ? 3 : 0;
}

}  // namespace

extern "C" {

// the plan of "combined" / "common" with every path; null: not a fixed shape
void* ff_new(const char* name) {
    Ff* f = new Ff();
    if (build(*f, name) != 0) { delete f; return nullptr; }
    return f;
}
void ff_free(void* h) { delete (Ff*)h; }
int ff_shape(void* h) { return ((Ff*)h)->shape; }
int ff_limit(int which) {
    return which == 0 ? 64 * ff::HEAD_WORDS : which == 1 ? 64 * ff::TAIL_WORDS : which == 2 ? ff::NUM_BYTES : ff::STATUS_BYTES;
}

int64_t ff_run(void* h, const uint8_t* buf, int64_t n, int off, int64_t* stats, uint8_t* flags, char* first, int cap) {
    std::string why;
    const int64_t bad = run(*(Ff*)h, buf, n, off, stats, flags, &why);
    if (first && cap) snprintf(first, (size_t)cap, "%s", why.c_str());
    return bad;
}

}  // extern "C"

#if defined(FF_MAIN)
// fixed_fast_emu_san SHAPE-NAME CORPUS-FILE: every line of the file at every
// window offset (built with -fsanitize=address,undefined and run directly).
int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s combined|common corpus-file\n", argv[0]); return 2; }
    Ff f;
    const int rc = build(f, argv[1]);
    if (rc) { fprintf(stderr, "%s: %s (%d)\n", argv[1], f.err.c_str(), rc); return rc; }
    FILE* fp = fopen(argv[2], "rb");
    if (!fp) { perror(argv[2]); return 2; }
    std::vector<uint8_t> data;
    uint8_t chunk[65536];
    for (size_t k; (k = fread(chunk, 1, sizeof chunk, fp)) > 0;) data.insert(data.end(), chunk, chunk + k);
    fclose(fp);
    int64_t stats[8];
    std::string why;
    const int64_t bad = run(f, data.data(), (int64_t)data.size(), -2, stats, nullptr, &why);
    printf("%s: %lld line views, %lld differ, %lld fast, %lld walked, %lld offset-dependent (ok %lld bad %lld fallback %lld redo %lld)\n",
           argv[1], (long long)stats[0], (long long)bad, (long long)stats[1], (long long)stats[2], (long long)stats[7],
           (long long)stats[3], (long long)stats[4], (long long)stats[5], (long long)stats[6]);
    if (bad) fprintf(stderr, "%s\n", why.c_str());
    return bad || stats[7] ? 1 : 0;
}
#endif
