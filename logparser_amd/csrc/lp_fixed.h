// Fixed LogFormat shapes: the compiled Program of a few very common
// LogFormats as compile-time constants.  The parse kernel has one instance
// per shape (parse_fixed.hip) in which the first-leaf walk is unrolled over
// these elements and the token-flag, time and first-line stages read their
// lists from here, so that the hot path loads no element descriptor, literal
// byte or stage entry from the Program and takes no branch on one.
//
// The tables only restate what lp_compile (plan.cpp compile_program) makes
// of the format with every path requested; the host picks an instance only
// when the handle's Program equals the table field by field
// (fixed_shape_of), so a table that drifted from plan.cpp selects nothing
// (tests/test_fixed_shape.py checks they agree).  A further shape is one
// more case in fixed_shape(); add none without a measurement.
#pragma once
#include "lp_program.h"

namespace lp {

enum : int { FS_NONE = 0, FS_COMBINED = 1, FS_COMMON = 2, FS_COUNT = 3 };
constexpr int FS_MAX_ELEMS = 24;

struct FixedShape {
    int n_elems = 0;
    int n_tok = 0;      // Program::n_tok
    int apache = 0;     // Program::fmt_apache[0]
    int n_time = 0;     // Program::n_time, every stage TK_APACHE on token time_tok[t]
    int time_tok[MAX_TIME] = {};
    int n_fl = 0;       // Program::n_fl, stage f on token fl_tok[f]
    int fl_tok[MAX_FL] = {};
    ElemV elems[FS_MAX_ELEMS] = {};
};

namespace fs {
constexpr int ACLS_QUOTE = 0;  // MC_QUOTE (lp_device.h), the mask class of '"'
constexpr int len(const char* s) { int n = 0; while (s[n]) ++n; return n; }
constexpr uint32_t lit4(const char* s) {
    uint32_t v = 0;
    for (int k = 0; k < 4 && s[k]; ++k) v |= (uint32_t)(uint8_t)s[k] << (8 * k);
    return v;
}
// a literal separator (at most 4 bytes: lit_at then compares lit4 alone)
constexpr ElemV lit(const char* s) { return ElemV{EK_LIT, 0, -1, 0, 0, len(s), 0, 0, -1, lit4(s)}; }
// a token captured in slot cap and followed by the literal `next`
constexpr ElemV tok(int kind, int cap, int det, const char* next, int need = 0) {
    return ElemV{kind, det, cap, 0, 0, len(next), 1, need, next[0] == '"' ? ACLS_QUOTE : -1, lit4(next)};
}
// the format's last token (followed by '$')
constexpr ElemV end(int kind, int cap) { return ElemV{kind, 1, cap, 1, 0, 0, 0, 0, -1, 0}; }
// literal pool offsets as compile_program hands them out: the literals one
// after the other, a token carries its following literal's
constexpr void offsets(FixedShape& S) {
    int off = 0;
    for (int i = 0; i < S.n_elems; ++i)
        if (S.elems[i].kind == EK_LIT) {
            S.elems[i].lit_off = off;
            off += S.elems[i].lit_len;
        }
    for (int i = 0; i + 1 < S.n_elems; ++i)
        if (S.elems[i].kind != EK_LIT && S.elems[i].nlit) S.elems[i].lit_off = S.elems[i + 1].lit_off;
}
}  // namespace fs

__host__ __device__ constexpr FixedShape fixed_shape(int shape) {
    FixedShape S{};
    int n = 0;
    switch (shape) {
    case FS_COMBINED:  // %h %l %u %t "%r" %>s %b "%{Referer}i" "%{User-Agent}i"
        S.elems[n++] = fs::tok(EK_NOSPACE, 0, 1, " ");
        S.elems[n++] = fs::lit(" ");
        S.elems[n++] = fs::tok(EK_CLFNUMBER, 1, 1, " ");
        S.elems[n++] = fs::lit(" ");
        S.elems[n++] = fs::tok(EK_NOSPACE, 2, 1, " [");
        S.elems[n++] = fs::lit(" [");
        S.elems[n++] = fs::tok(EK_TIME_US, 3, 1, "] \"");
        S.elems[n++] = fs::lit("] \"");
        S.elems[n++] = fs::tok(EK_ANY_GREEDY, 4, 0, "\" ", 5);  // '"' bytes of the literals after it
        S.elems[n++] = fs::lit("\" ");
        S.elems[n++] = fs::tok(EK_NOSPACE, 5, 1, " ");
        S.elems[n++] = fs::lit(" ");
        S.elems[n++] = fs::tok(EK_CLFNUMBER, 6, 1, " \"");
        S.elems[n++] = fs::lit(" \"");
        S.elems[n++] = fs::tok(EK_ANY_LAZY, 7, 0, "\" \"");
        S.elems[n++] = fs::lit("\" \"");
        S.elems[n++] = fs::tok(EK_ANY_LAZY, 8, 0, "\"");
        S.elems[n++] = fs::lit("\"");
        S.n_tok = 9;
        break;
    case FS_COMMON:  // %h %l %u %t "%r" %>s %b
        S.elems[n++] = fs::tok(EK_NOSPACE, 0, 1, " ");
        S.elems[n++] = fs::lit(" ");
        S.elems[n++] = fs::tok(EK_CLFNUMBER, 1, 1, " ");
        S.elems[n++] = fs::lit(" ");
        S.elems[n++] = fs::tok(EK_NOSPACE, 2, 1, " [");
        S.elems[n++] = fs::lit(" [");
        S.elems[n++] = fs::tok(EK_TIME_US, 3, 1, "] \"");
        S.elems[n++] = fs::lit("] \"");
        S.elems[n++] = fs::tok(EK_ANY_GREEDY, 4, 0, "\" ", 1);
        S.elems[n++] = fs::lit("\" ");
        S.elems[n++] = fs::tok(EK_NOSPACE, 5, 1, " ");
        S.elems[n++] = fs::lit(" ");
        S.elems[n++] = fs::end(EK_CLFNUMBER, 6);
        S.n_tok = 7;
        break;
    default: return S;
    }
    S.n_elems = n;
    S.apache = 1;
    S.n_time = 1;
    S.time_tok[0] = 3;  // %t
    S.n_fl = 1;
    S.fl_tok[0] = 4;    // %r
    fs::offsets(S);
    return S;
}

// The shape whose instance may parse P: every field the instance treats as a
// constant equals P's, and P is a SIMPLE program (capi simple_program: the
// instance is built on the SIMPLE one).  FS_NONE: today's instances.
inline bool fixed_shape_equals(const FixedShape& S, const Program& P) {
    if (P.n_fmt != 1 || P.n_elems != S.n_elems || P.fmt_elem0[0] != 0 || P.fmt_elem0[1] != S.n_elems) return false;
    if (P.n_tok != S.n_tok || (P.fmt_apache[0] != 0) != (S.apache != 0)) return false;
    if (P.n_secms || P.n_binip || P.guard_pct[0] || P.guard_setc[0]) return false;
    if (P.n_time != S.n_time || P.n_fl != S.n_fl) return false;
    for (int t = 0; t < S.n_time; ++t)
        if (P.time[t].tok != S.time_tok[t] || P.time[t].fmt != 0 || P.time[t].kind != TK_APACHE) return false;
    for (int f = 0; f < S.n_fl; ++f)
        if (P.fl[f].tok != S.fl_tok[f] || P.fl[f].fmt != 0) return false;
    for (int i = 0; i < S.n_elems; ++i) {
        const ElemV a = load_elem(P.elems + i), b = S.elems[i];
        if (a.kind != b.kind || a.det != b.det || a.cap != b.cap || a.last != b.last || a.lit_off != b.lit_off ||
            a.lit_len != b.lit_len || a.nlit != b.nlit || a.need != b.need || a.acls != b.acls || a.lit4 != b.lit4)
            return false;
        // the literal's bytes themselves (the instance compares lit4 only)
        if (b.lit_len > 4 || b.lit_off + b.lit_len > MAX_LIT) return false;
        for (int k = 0; k < b.lit_len; ++k)
            if (P.lit[b.lit_off + k] != (uint8_t)(b.lit4 >> (8 * k))) return false;
    }
    return true;
}
inline int fixed_shape_of(const Program& P) {
    for (int s = 1; s < FS_COUNT; ++s)
        if (fixed_shape_equals(fixed_shape(s), P)) return s;
    return FS_NONE;
}

}  // namespace lp
