// TEST-ONLY CPU unit for the fixed-shape instances of the parse kernel
// (logparser_amd/csrc/lp_fixed.h, lp_device.h match_fixed_leaf / phase1<...,
// SHAPE>), built to a library of its own (tests/fixed_emu_lib.py) and, with
// -DFX_MAIN, to a stand-alone program that runs the adversarial set under
// the sanitizers.  It checks three things:
//   table drift    the Program plan.cpp compiles from a format name against
//                  the shape's constant table, field by field, and the
//                  host's predicate (fixed_shape_of) on near-miss formats
//   differential   match_fixed_leaf<SHAPE> against match_first_leaf<LA, SIMPLE>
//                  (boolean and capture spans), and the whole phase 1 of the
//                  fixed instance against the SIMPLE instance's, on line
//                  views with and without mask planes, the line at a chosen
//                  offset of its 64-byte window
//   adversarial    the set of hostile lines built from a valid line of a
//                  shape (fx_adv_*), shared with the GPU tests
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../logparser_amd/csrc/lp_device.h"
#include "../../logparser_amd/csrc/plan.h"

using namespace lp;

namespace {

struct Fx {
    Plan plan;
    std::string err;
};

const char* kValid[FS_COUNT] = {
    "",
    "203.0.113.7 - frank [10/Oct/2026:13:55:36 -0700] \"GET /apache_pb.gif?a=1&b=2 HTTP/1.1\" 200 2326 "
    "\"http://www.example.com/start.html?q=x\" \"Mozilla/5.0 (X11; Linux x86_64) Gecko/20100101 Firefox/115.0\"",
    "203.0.113.7 - frank [10/Oct/2026:13:55:36 -0700] \"GET /apache_pb.gif?a=1&b=2 HTTP/1.1\" 200 2326",
};

template <int SHAPE, typename LN>
bool leaf_pair(const Program& P, const LN& L, std::string* why) {
    RegArr<MAX_TOK> a, b;
    a.fill(0);
    b.fill(0);
    const bool ra = match_first_leaf<false, true>(P, L, a);
    const bool rb = match_fixed_leaf<SHAPE, false>(P, L, b);
    bool same = ra == rb;
    for (int k = 0; k < MAX_TOK; ++k) same = same && a.v[k] == b.v[k];
    if (!same && why) *why = "first leaf: generic " + std::to_string(ra) + " fixed " + std::to_string(rb);
    return same;
}

bool same_out(const LineOut& x, const LineOut& y, std::string* why) {
    auto arr = [&](const char* name, const uint32_t* p, const uint32_t* q, int n) {
        for (int k = 0; k < n; ++k)
            if (p[k] != q[k]) {
                if (why) *why = std::string("phase 1: ") + name + "[" + std::to_string(k) + "]";
                return false;
            }
        return true;
    };
    if (x.status != y.status) {
        if (why) *why = "phase 1: status " + std::to_string(x.status) + " / " + std::to_string(y.status);
        return false;
    }
    if (x.status != ST_OK) return true;  // (a line that is not OK delivers nothing else)
    if (x.tok_flags != y.tok_flags || x.tdone != y.tdone || x.hist != y.hist) {
        if (why) *why = "phase 1: tok_flags / tdone / hist";
        return false;
    }
    return arr("caps", x.caps.v, y.caps.v, MAX_TOK) && arr("fl_kind", x.fl_kind.v, y.fl_kind.v, MAX_FL) &&
           arr("fl_method", x.fl_method.v, y.fl_method.v, MAX_FL) && arr("fl_uri", x.fl_uri.v, y.fl_uri.v, MAX_FL) &&
           arr("fl_proto", x.fl_proto.v, y.fl_proto.v, MAX_FL) && arr("ep_lo", x.ep_lo.v, y.ep_lo.v, MAX_TIME) &&
           arr("ep_hi", x.ep_hi.v, y.ep_hi.v, MAX_TIME) && arr("lo_lo", x.lo_lo.v, y.lo_lo.v, MAX_TIME) &&
           arr("lo_hi", x.lo_hi.v, y.lo_hi.v, MAX_TIME) && arr("ut_lo", x.ut_lo.v, y.ut_lo.v, MAX_TIME) &&
           arr("ut_hi", x.ut_hi.v, y.ut_hi.v, MAX_TIME) && arr("nano", x.nano.v, y.nano.v, MAX_TIME);
}

// the chunk kernel's phase 1 (no DFS: ST_REDO) of the SIMPLE instance and of the fixed one
template <int SHAPE, typename LN>
bool phase1_pair(const Program& P, const LN& L, int* status, std::string* why) {
    Columns C;
    memset(&C, 0, sizeof C);
    uint32_t stk[MAX_STACK];
    LineOut x, y;
    memset(&x, 0, sizeof x);
    memset(&y, 0, sizeof y);
    phase1<false, false, true, false>(P, P.elems, L, x, stk, C, 0, false, 0);
    phase1<false, false, true, false, false, SHAPE>(P, P.elems, L, y, stk, C, 0, false, 0);
    *status = x.status;
    return same_out(x, y, why);
}

// One line at byte `off` (0..63) of a 64-byte aligned window whose other
// bytes are quotes, spaces and a terminator, as neighbouring lines would
// leave them (so bits 63 and 0 of the mask words next to the line are set).
template <int SHAPE>
bool diff_line(const Program& P, const uint8_t* line, int n, int off, int* status, std::string* why) {
    const uint32_t wn = (uint32_t)((off + n + 1 + 8 + 63) & ~63);
    std::vector<uint64_t> wbuf(wn / 8 + 8, 0);
    uint8_t* w = (uint8_t*)wbuf.data();
    static const char fill[] = "\" \"x ";
    for (uint32_t k = 0; k < wn + 64; ++k) w[k] = (uint8_t)fill[k % 5];
    if (off) w[off - 1] = '\n';
    memcpy(w + off, line, (size_t)n);
    w[off + n] = '\n';
    std::vector<uint64_t> masks(MC_N * (wn / 64));
    build_masks(w, wn, masks.data());
    const MLine M{w, (uint32_t)off, n, masks.data()};
    const Line S{w, (uint32_t)off, n};
    int st2 = 0;
    if (!leaf_pair<SHAPE>(P, M, why) || !leaf_pair<SHAPE>(P, S, why)) return false;
    if (!phase1_pair<SHAPE>(P, M, status, why) || !phase1_pair<SHAPE>(P, S, &st2, why)) return false;
    if (*status != st2) {
        if (why) *why = "mask / SWAR views disagree";
        return false;
    }
    return true;
}

bool diff_line_shape(int shape, const Program& P, const uint8_t* line, int n, int off, int* status, std::string* why) {
    switch (shape) {
    case FS_COMBINED: return diff_line<FS_COMBINED>(P, line, n, off, status, why);
    case FS_COMMON: return diff_line<FS_COMMON>(P, line, n, off, status, why);
    }
    if (why) *why = "no such shape";
    return false;
}

// ---- the adversarial set of a shape, from its valid line
std::vector<std::string> adversarial(int shape) {
    const FixedShape S = fixed_shape(shape);
    const std::string v = kValid[shape];
    std::vector<std::string> out;
    out.push_back(v);
    // element spans of the valid line: tokens by their literals, in order
    std::vector<std::pair<int, int>> span(S.n_elems);
    {
        int pos = 0;
        for (int i = 0; i < S.n_elems; ++i) {
            const ElemV e = S.elems[i];
            if (e.kind == EK_LIT) {
                span[i] = {pos, pos + e.lit_len};
                pos += e.lit_len;
            } else {
                int end = (int)v.size();
                if (e.nlit) {
                    std::string lit;
                    for (int k = 0; k < e.lit_len; ++k) lit.push_back((char)(e.lit4 >> (8 * k)));
                    // (the valid line's tokens do not hold their following literal)
                    end = (int)v.find(lit, (size_t)pos);
                }
                span[i] = {pos, end};
                pos = end;
            }
        }
    }
    for (int i = 0; i < S.n_elems; ++i) {
        const ElemV e = S.elems[i];
        const int a = span[i].first, b = span[i].second;
        if (e.kind == EK_LIT) {
            // every literal with one byte changed, one at a time
            for (int k = a; k < b; ++k)
                for (char c : {'X', '\t', '"', ' ', '-'})
                    if (v[k] != c) { std::string s = v; s[k] = c; out.push_back(s); }
            // ... and with one byte dropped or doubled
            for (int k = a; k < b; ++k) {
                out.push_back(v.substr(0, k) + v.substr(k + 1));
                out.push_back(v.substr(0, k) + v[k] + v.substr(k));
            }
            continue;
        }
        // the following literal's bytes (and pieces of the quoted ones) planted inside the token
        for (const char* plant : {"\"", "\" ", "\" \"", "\\\"", " ", " [", "] \"", " \"", "]", "["})
            for (int at : {a, (a + b) / 2, b}) out.push_back(v.substr(0, at) + plant + v.substr(at));
        // empty and "-" tokens
        out.push_back(v.substr(0, a) + v.substr(b));
        out.push_back(v.substr(0, a) + "-" + v.substr(b));
        out.push_back(v.substr(0, a) + "0" + v.substr(b));
    }
    // TAB for a space, one at a time
    for (size_t k = 0; k < v.size(); ++k)
        if (v[k] == ' ') { std::string s = v; s[k] = '\t'; out.push_back(s); }
    // the line cut at every length, and with bytes appended
    for (size_t k = 0; k < v.size(); ++k) out.push_back(v.substr(0, k));
    for (const char* tail : {" ", "\"", " x", "\" \"x\"", " \"-\"", "\t", " -"}) out.push_back(v + tail);
    // lengths around MAX_LINE (the last token padded)
    for (int n : {MAX_LINE - 1, MAX_LINE, MAX_LINE + 1}) {
        const int last = S.elems[S.n_elems - 1].kind == EK_LIT ? S.n_elems - 2 : S.n_elems - 1;
        const int at = span[last].second;
        const char pad = S.elems[last].kind == EK_CLFNUMBER ? '7' : 'a';
        out.push_back(v.substr(0, at) + std::string((size_t)(n - (int)v.size()), pad) + v.substr(at));
    }
    return out;
}

const std::vector<std::string>& adv_set(int shape) {
    static std::vector<std::string> sets[FS_COUNT];
    if (shape <= 0 || shape >= FS_COUNT) return sets[0];
    if (sets[shape].empty()) sets[shape] = adversarial(shape);
    return sets[shape];
}

}  // namespace

extern "C" {

// the plan of a logformat with the given fields; null: it did not compile
void* fx_new(const char* fmt, const char* const* fields, int n, char* err, int errlen) {
    Fx* f = new Fx();
    std::vector<std::string> fl(fields, fields + n);
    const int st = f->plan.build(fmt, fl, f->err);
    if (err && errlen) snprintf(err, (size_t)errlen, "%s", f->err.c_str());
    if (st != 0) { delete f; return nullptr; }
    return f;
}
void fx_free(void* h) { delete (Fx*)h; }

// the host's predicate (capi.cpp picks the instance with it)
int fx_shape_of(void* h) {
    Fx* f = (Fx*)h;
    return f->plan.device_ok() ? fixed_shape_of(f->plan.program()) : FS_NONE;
}

// the compiled Program against the shape's table, field by field: the
// number of fields that differ, their names in out
int fx_table_diff(void* h, int shape, char* out, int cap) {
    const Program& P = ((Fx*)h)->plan.program();
    const FixedShape S = fixed_shape(shape);
    std::string d;
    int n = 0;
    auto chk = [&](const std::string& name, long a, long b) {
        if (a == b) return;
        ++n;
        d += name + " program " + std::to_string(a) + " table " + std::to_string(b) + "\n";
    };
    chk("n_fmt", P.n_fmt, 1);
    chk("n_elems", P.n_elems, S.n_elems);
    chk("n_tok", P.n_tok, S.n_tok);
    chk("apache", P.fmt_apache[0], S.apache);
    chk("n_time", P.n_time, S.n_time);
    chk("n_fl", P.n_fl, S.n_fl);
    for (int t = 0; t < S.n_time && t < P.n_time; ++t) {
        chk("time.tok", P.time[t].tok, S.time_tok[t]);
        chk("time.kind", P.time[t].kind, TK_APACHE);
        chk("time.fmt", P.time[t].fmt, 0);
    }
    for (int k = 0; k < S.n_fl && k < P.n_fl; ++k) {
        chk("fl.tok", P.fl[k].tok, S.fl_tok[k]);
        chk("fl.fmt", P.fl[k].fmt, 0);
    }
    for (int i = 0; i < S.n_elems && i < P.n_elems; ++i) {
        const ElemV a = load_elem(P.elems + i), b = S.elems[i];
        const std::string e = "elem " + std::to_string(i) + " ";
        chk(e + "kind", a.kind, b.kind);
        chk(e + "det", a.det, b.det);
        chk(e + "cap", a.cap, b.cap);
        chk(e + "last", a.last, b.last);
        chk(e + "lit_off", a.lit_off, b.lit_off);
        chk(e + "lit_len", a.lit_len, b.lit_len);
        chk(e + "nlit", a.nlit, b.nlit);
        chk(e + "need", a.need, b.need);
        chk(e + "acls", a.acls, b.acls);
        chk(e + "lit4", (long)a.lit4, (long)b.lit4);
        for (int k = 0; k < b.lit_len && k < 4; ++k) chk(e + "lit byte", P.lit[a.lit_off + k], (uint8_t)(b.lit4 >> (8 * k)));
    }
    chk("predicate", fixed_shape_equals(S, P) ? 1 : 0, n == 0 ? 1 : 0);
    if (out && cap) snprintf(out, (size_t)cap, "%s", d.c_str());
    return n;
}

// Differential of every '\n'-terminated line of buf[0, n) at window offset
// off (0..63; < 0: line i at offset i mod 64): the lines on which the fixed
// instance and the generic one differ.  stats: [0] lines, [1] OK, [2] BAD,
// [3] FALLBACK, [4] REDO.  first: the first differing line's number and why.
int64_t fx_diff(void* h, int shape, const uint8_t* buf, int64_t n, int off, int64_t* stats, char* first, int cap) {
    const Program& P = ((Fx*)h)->plan.program();
    int64_t bad = 0, i = 0;
    for (int k = 0; k < 5; ++k) stats[k] = 0;
    for (int64_t s = 0; s < n; ++i) {
        const uint8_t* nl = (const uint8_t*)memchr(buf + s, '\n', (size_t)(n - s));
        const int64_t e = nl ? nl - buf : n;
        int st = 0;
        std::string why;
        if (!diff_line_shape(shape, P, buf + s, (int)(e - s), off < 0 ? (int)(i & 63) : off, &st, &why)) {
            if (!bad++ && first && cap) snprintf(first, (size_t)cap, "line %lld: %s", (long long)i, why.c_str());
        }
        ++stats[0];
        if (st >= 0 && st <= 3) ++stats[1 + st];
        s = e + 1;
    }
    return bad;
}

// the adversarial set of a shape
int fx_adv_count(int shape) { return (int)adv_set(shape).size(); }
int fx_adv_get(int shape, int i, char* out, int cap) {
    const std::string& s = adv_set(shape)[(size_t)i];
    if ((int)s.size() > cap) return -1;
    memcpy(out, s.data(), s.size());
    return (int)s.size();
}

}  // extern "C"

#if defined(FX_MAIN)
// The adversarial set of both shapes, every line at every window offset,
// through the host build of both matchers (built with -fsanitize=address,undefined
// by tests/test_fixed_shape.py and run directly).
int main() {
    static const char* names[FS_COUNT] = {"", "combined", "common"};
    int rc = 0;
    for (int shape = 1; shape < FS_COUNT; ++shape) {
        Fx f;
        std::vector<std::string> paths;
        if (Plan::possible_paths(names[shape], 15, paths, f.err) != 0 || f.plan.build(names[shape], paths, f.err) != 0) {
            fprintf(stderr, "%s does not compile: %s\n", names[shape], f.err.c_str());
            return 2;
        }
        if (fixed_shape_of(f.plan.program()) != shape) {
            fprintf(stderr, "%s: not the fixed shape\n", names[shape]);
            return 3;
        }
        long lines = 0, differ = 0, by_status[4] = {0, 0, 0, 0};
        for (const std::string& s : adv_set(shape))
            for (int off = 0; off < 64; ++off) {
                int st = 0;
                std::string why;
                ++lines;
                if (!diff_line_shape(shape, f.plan.program(), (const uint8_t*)s.data(), (int)s.size(), off, &st, &why)) {
                    if (!differ++) fprintf(stderr, "%s: %s\n  %s\n", names[shape], why.c_str(), s.substr(0, 300).c_str());
                }
                if (st >= 0 && st <= 3) ++by_status[st];
            }
        printf("%s: %ld line views, %ld differ (ok %ld bad %ld fallback %ld redo %ld)\n", names[shape], lines, differ,
               by_status[0], by_status[1], by_status[2], by_status[3]);
        if (differ) rc = 1;
    }
    return rc;
}
#endif
