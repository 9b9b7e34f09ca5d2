// One row's value of one table column on the device: what the planner's
// TableSrc (lp_table.h) names, read from the parse kernels' SoA columns.
// Shared by the kernel units of the typed table (table.hip) and of its
// dictionary-encoded columns (dict.hip); each unit gets its own copy in its
// anonymous namespace.  Include after kernels.h and lp_device.h, in a unit
// that defines LP_KERNEL_TU.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "lp_device.h"
#include "lp_geoip.h"  // GeoField, geo_slot (TC_GEOIP)
#include "lp_value.h"  // digits, write_long, parse_long, decimal_to_double

namespace lp {

namespace {

// one value: 0 none (null / not delivered), 1 bytes at p (amp: a '&' first),
// 2 a long, 3 bytes in buf
struct TVal {
    int kind = 0;
    const LP_G uint8_t* p = nullptr;
    uint32_t n = 0;
    bool amp = false;
    int64_t l = 0;
    char buf[20];  // formatted values (dates, times, month names, binary IPs)
};

__constant__ char MONTH_TEXT[] = "JanuaryFebruaryMarchAprilMayJuneJulyAugustSeptemberOctoberNovemberDecember";
__constant__ uint8_t MONTH_OFF[13] = {0, 7, 15, 20, 25, 28, 32, 36, 42, 51, 58, 66, 74};

__device__ __forceinline__ void put2(char* b, int64_t v) {
    b[0] = (char)('0' + v / 10);
    b[1] = (char)('0' + v % 10);
}

// ResponseSetCookieDissector.dissect (dissectors/ResponseSetCookieDissector.java:86-135) on one
// cookie string [cp, cp + cn) -- the cookie's LAST cookie string (every
// dissection of a name reads the Parsable's cached last value,
// core/Parsable.java:172-183): split(";"), each part trimmed and split("=", 2),
// key and value trimmed; part 0's value is "value", a later part keyed
// "expires" / "domain" / "comment" / "path" delivers that output (the last such
// part wins, ParsedRecord).  Out of line: the table kernels' other columns
// keep their registers.  kind / p / n / l as TVal.
__device__ __noinline__ void setcookie_attr(const LP_G uint8_t* cp, uint32_t cn, int fld, int& kind,
                                            const LP_G uint8_t*& p, uint32_t& n, int64_t& l) {
    auto pk = [](const char* k) {
        uint64_t x = 0;
        for (int q = 0; k[q]; ++q) x |= (uint64_t)(uint8_t)k[q] << (8 * q);
        return x;
    };
    const uint64_t want = fld == SC_DOMAIN ? pk("domain") : fld == SC_COMMENT ? pk("comment") : fld == SC_PATH ? pk("path")
                                                                                                    : pk("expires");
    const uint32_t klen = fld == SC_DOMAIN ? 6u : fld == SC_COMMENT ? 7u : fld == SC_PATH ? 4u : 7u;
    for (uint32_t ps = 0, part = 0; ps <= cn; ++part) {
        uint32_t pe = ps;
        while (pe < cn && cp[pe] != ';') ++pe;
        uint32_t a = ps, b = pe;
        while (a < b && cp[a] <= ' ') ++a;
        while (b > a && cp[b - 1] <= ' ') --b;
        uint32_t x = a;
        while (x < b && cp[x] != '=') ++x;
        uint32_t ka = a, kb = x, va = x < b ? x + 1 : b, vb = b;
        while (kb > ka && cp[kb - 1] <= ' ') --kb;
        while (va < vb && cp[va] <= ' ') ++va;
        if (part == 0) {
            if (fld == SC_VALUE) { kind = 1; p = cp + va; n = vb - va; }
        } else if (fld != SC_VALUE && kb - ka == klen) {
            uint64_t k = 0;
            for (uint32_t q = 0; q < klen; ++q) k |= (uint64_t)cp[ka + q] << (8 * q);
            if (k == want) {
                if (fld == SC_EXPIRES_S || fld == SC_EXPIRES_MS) {
                    // parseExpire: "EEE, dd-MMM-yyyy HH:mm:ss GMT" (the only layout the
                    // phase-1 guard lets through) -> epoch seconds * 1000; STRING:expires
                    // is that / 1000 (ResponseSetCookieDissector.java:104-107, 137-150)
                    const LP_G uint8_t* d = cp + va;
                    int mon = 1;
                    for (int q = 0; q < 12; ++q)
                        if (d[8] == (uint8_t)MONTH_TEXT[MONTH_OFF[q]] && d[9] == (uint8_t)MONTH_TEXT[MONTH_OFF[q] + 1] &&
                            d[10] == (uint8_t)MONTH_TEXT[MONTH_OFF[q] + 2])
                            mon = q + 1;
                    auto d2 = [&](int q) { return (int)(d[q] - '0') * 10 + (int)(d[q + 1] - '0'); };
                    const int64_t days = days_from_civil(d2(12) * 100 + d2(14), mon, d2(5));
                    const int64_t ms = (days * 86400 + d2(17) * 3600 + d2(20) * 60 + d2(23)) * 1000;
                    kind = 2;
                    l = fld == SC_EXPIRES_S ? ms / 1000 : ms;
                } else {
                    kind = 1;
                    p = cp + va;
                    n = vb - va;
                }
            }
        }
        ps = pe + 1;
    }
}

// A re-dissected remapped value (lp_program.h ValStage; TC_SCREEN / TC_UNIQUEID)
// on the located value [sp, sp + sn): ScreenResolutionDissector's width / height
// as a sub-span of the value (the line, or the decoded value in the region),
// ModUniqueIdDissector's fields as longs, its address formatted into buf
// (lp_value.h screen_split / unique_id_decode).  Out of line, as
// setcookie_attr: the other columns keep their registers.  kind / p / n / l
// as TVal.
__device__ __noinline__ void remap_value(int tc, int fld, const LP_G uint8_t* sp, uint32_t sn, int& kind,
                                         const LP_G uint8_t*& p, uint32_t& n, int64_t& l, char* buf) {
    if (tc == TC_SCREEN) {
        uint32_t wl, ho, hl;
        const int parts = screen_split(sp, sn, wl, ho, hl);
        if (parts <= fld) return;  // no 'x', or (not on an OK line: the guard of derived_line) a missing part
        kind = 1;
        p = fld ? sp + ho : sp;
        n = fld ? hl : wl;
        return;
    }
    uint32_t f[5];
    if (!unique_id_decode(sp, sn, f)) return;
    if (fld == UQ_IP) {
        kind = 3;
        n = unique_id_ip(f[1], buf);
        return;
    }
    kind = 2;
    l = fld == UQ_EPOCH ? (int64_t)f[0] * 1000 : fld == UQ_PROCESSID ? (int64_t)f[2] : fld == UQ_COUNTER ? (int64_t)f[3]
                                                                                                          : (int64_t)f[4];
}

// A GeoIP output (TC_GEOIP): a gather from the stage's field table (lp_geoip.h
// GeoField as two u64: v; off | len << 32) through the line's record id + 1
// (rec; 0: a null / empty address, or one that is not in the tree -- no
// outputs).  A LONG field is its value; a STRING its bytes in the pool; a
// DOUBLE its text in the pool with the f64's bits in l (for a DOUBLE column).
// Out of line, as remap_value.  kind / p / n / l as TVal.
__device__ __noinline__ void geo_value(const Columns& C, int32_t want, const TableSrc& s, int64_t i, int& kind,
                                       const LP_G uint8_t*& p, uint32_t& n, int64_t& l) {
    const uint32_t rec = C.geo[s.a][i];
    if (rec == 0) return;
    const LP_G uint64_t* f = C.geo_fields[s.a] + 2 * ((size_t)geo_slot((uint32_t)want, s.b) * C.geo_records[s.a] + (rec - 1));
    const uint64_t w1 = f[1];
    if ((uint32_t)w1 == GEO_NULL) return;
    l = (int64_t)f[0];
    if (s.c == GK_LONG) {
        kind = 2;
    } else {
        kind = 1;
        p = C.geo_pool[s.a] + (uint32_t)w1;
        n = (uint32_t)(w1 >> 32);
    }
}

__device__ TVal tvalue(const Program& P, const Columns& C, const TableArgs& T, const TableSrc& s, int64_t i,
                       const LP_G uint8_t* line, const LP_G uint8_t* region) {
    TVal v;

    auto bytes = [&](const LP_G uint8_t* p, uint32_t n) {
        v.kind = 1;
        v.p = p;
        v.n = n;
    };
    auto span = [&](uint32_t sp) { bytes(line + (sp & 0xFFFFu), (sp >> 16) - (sp & 0xFFFFu)); };
    auto ref = [&](uint64_t r) {
        bytes((ref_arena(r) ? region : line) + ref_off(r), ref_len(r));
        v.amp = ref_amp(r);
    };
    auto along = [&](int64_t l) {
        v.kind = 2;
        v.l = l;
    };
    switch (s.kind) {
    case TC_TOKEN: case TC_CLF2NUM: case TC_NUM2CLF: {
        const bool null = (C.tok_flags[i] >> s.a) & 1u;
        if (null) {
            if (s.kind == TC_CLF2NUM) along(0);  // ConvertCLFIntoNumber: null -> 0L
            return v;
        }
        span(C.tok_span[s.a][i]);
        if (s.kind == TC_NUM2CLF && v.n == 1 && v.p[0] == '0') v.kind = 0;  // "0" -> null
        return v;
    }
    case TC_TIME: {
        const TimeStage& TS = P.time[s.a];
        const uint32_t sp = C.tok_span[TS.tok][i];
        if (((C.tok_flags[i] >> TS.tok) & 1u) || (sp >> 16) <= (sp & 0xFFFFu)) return v;  // null / empty: no dissection
        if (s.b == TF_EPOCH) { along(C.t_epoch[s.a][i]); return v; }
        const uint64_t w = s.c ? C.t_utc[s.a][i] : C.t_local[s.a][i];
        const int64_t Y = w & 0xFFFF, MO = (w >> 16) & 15, D = (w >> 20) & 31, H = (w >> 25) & 31, MI = (w >> 30) & 63,
                      S = (w >> 36) & 63, WY = (w >> 42) & 0xFFFF, WK = (w >> 58) & 63;
        const int64_t nanos = TS.kind == TK_STRF ? (int64_t)C.t_nano[s.a][i] : 0;
        switch (s.b) {
        case TF_DAY: along(D); break;
        case TF_MONTH: along(MO); break;
        case TF_WEEK: along(WK); break;
        case TF_WEEKYEAR: along(WY); break;
        case TF_YEAR: along(Y); break;
        case TF_HOUR: along(H); break;
        case TF_MINUTE: along(MI); break;
        case TF_SECOND: along(S); break;
        case TF_MILLI: along(nanos / 1000000); break;
        case TF_MICRO: along(nanos / 1000); break;
        case TF_NANO: along(nanos); break;
        case TF_MONTHNAME:
            v.kind = 3;
            v.n = MONTH_OFF[MO] - MONTH_OFF[MO - 1];
            for (uint32_t k = 0; k < v.n; ++k) v.buf[k] = MONTH_TEXT[MONTH_OFF[MO - 1] + k];
            break;
        case TF_DATE: {  // "%04d-%02d-%02d", as Plan::replay prints it: a packed year past 9999 (none comes
            // from the parse kernels: time_fields sends such a line to FALLBACK) takes five digits
            const uint32_t o = Y > 9999 ? 1u : 0u;
            v.kind = 3;
            v.n = 10 + o;
            v.buf[0] = (char)('0' + Y / 10000);
            put2(v.buf + o, Y / 100 % 100);
            put2(v.buf + o + 2, Y % 100);
            v.buf[o + 4] = '-';
            put2(v.buf + o + 5, MO);
            v.buf[o + 7] = '-';
            put2(v.buf + o + 8, D);
            break;
        }
        case TF_TIME:  // "%02d:%02d:%02d"
            v.kind = 3;
            v.n = 8;
            put2(v.buf, H);
            v.buf[2] = ':';
            put2(v.buf + 3, MI);
            v.buf[5] = ':';
            put2(v.buf + 6, S);
            break;
        default: break;
        }
        return v;
    }
    case TC_FL: {
        const uint32_t kind = C.fl_kind[s.a][i];
        if (kind == FL_NONE) return v;
        if (s.b == 0) span(C.fl_method[s.a][i]);
        else if (s.b == 1) span(C.fl_uri[s.a][i]);
        else if (kind == FL_FULL) span(C.fl_proto[s.a][i]);  // a chopped line's protocol is null
        return v;
    }
    case TC_PROTO: {  // HttpFirstLineProtocolDissector: "HTTP/x.y".split("/", 2)
        if (C.fl_kind[s.a][i] != FL_FULL) return v;
        span(C.fl_proto[s.a][i]);
        if (v.n == 0 || (v.n == 1 && v.p[0] == '-')) { v.kind = 0; return v; }
        uint32_t sl = 0;
        while (sl < v.n && v.p[sl] != '/') ++sl;
        if (sl == v.n) { v.kind = 0; return v; }  // no '/': both null
        if (s.b == 0) v.n = sl;
        else { v.p += sl + 1; v.n -= sl + 1; }
        return v;
    }
    case TC_URI: {
        const uint32_t f = C.u_flags[s.a][i];
        if (!(f & UF_DONE)) return v;
        switch (s.b) {
        case UP_QUERY: ref(C.u_query[s.a][i]); break;
        case UP_PATH: ref(C.u_path[s.a][i]); break;
        case UP_REF: if (f & UF_FRAG) ref(C.u_frag[s.a][i]); break;
        case UP_PROTOCOL: if ((f & UF_IS_URL) && (f & UF_SCHEME)) ref(C.u_scheme[s.a][i]); break;
        case UP_HOST: if ((f & UF_IS_URL) && (f & UF_HOST)) ref(C.u_host[s.a][i]); break;
        case UP_PORT: if ((f & UF_IS_URL) && (f & UF_PORT)) along(C.u_port[s.a][i]); break;
        default: break;
        }
        return v;
    }
    case TC_SECMS:  // ConvertSecondsWithMillisStringDissector (+ ConvertMillisecondsIntoMicroseconds)
        if (!((C.tok_flags[i] >> P.secms[s.a].tok) & 1u)) along(s.b ? (int64_t)((uint64_t)C.sm_ms[s.a][i] * 1000u) : C.sm_ms[s.a][i]);
        return v;
    case TC_BINIP: {  // BinaryIPDissector: "%d.%d.%d.%d" of the signed bytes
        const uint32_t sp = C.tok_span[P.binip[s.a].tok][i];
        if ((sp >> 16) - (sp & 0xFFFFu) != 16u) return v;
        const uint32_t x = C.bip[s.a][i];
        v.kind = 3;
        v.n = 0;
        for (int k = 0; k < 4; ++k) {
            int b = (int)(int8_t)((x >> (8 * k)) & 0xFF);
            if (k) v.buf[v.n++] = '.';
            if (b < 0) { v.buf[v.n++] = '-'; b = -b; }
            if (b >= 100) v.buf[v.n++] = (char)('0' + b / 100);
            if (b >= 10) v.buf[v.n++] = (char)('0' + (b / 10) % 10);
            v.buf[v.n++] = (char)('0' + b % 10);
        }
        return v;
    }
    case TC_LIST: case TC_LIST_MS: {  // UpstreamListDissector item b (its table in the line's region)
        if ((uint32_t)s.b >= C.l_count[s.a][i]) return v;
        const uint32_t ent = P.list[s.a].secms ? LIST_ENT_MS : LIST_ENT;
        const LP_G uint8_t* e = region + ref_off(C.l_tab[s.a][i]) + (uint32_t)s.b * ent;
        if (s.kind == TC_LIST) {
            span(reinterpret_cast<const LP_G uint32_t*>(e)[s.c & 1]);
        } else {
            const int64_t ms = reinterpret_cast<const LP_G int64_t*>(e + 8)[s.c & 1];
            along((s.c & 2) ? (int64_t)((uint64_t)ms * 1000u) : ms);
        }
        return v;
    }
    case TC_PAIR: {  // the cookie / parameter's last occurrence in the pair stage's piece table
        const uint32_t cnt = C.p_count[s.a][i];
        const LP_G uint64_t* t = reinterpret_cast<const LP_G uint64_t*>(region + ref_off(C.p_tab[s.a][i]));
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint64_t nref = t[2 * k];
            if (ref_len(nref) != (uint32_t)s.c) continue;
            const LP_G uint8_t* np = (ref_arena(nref) ? region : line) + ref_off(nref);
            bool same = true;
            for (int q = 0; q < s.c && same; ++q) same = np[q] == T.names[s.b + q];
            if (same) ref(t[2 * k + 1]);
        }
        return v;
    }
    case TC_SETC: {
        const int j = s.a & 0xFF;
        const uint32_t cnt = C.p_count[j][i];
        const LP_G uint64_t* t = reinterpret_cast<const LP_G uint64_t*>(region + ref_off(C.p_tab[j][i]));
        uint64_t cref = 0;
        bool found = false;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint64_t nref = t[2 * k];
            if (ref_len(nref) != (uint32_t)s.c) continue;
            const LP_G uint8_t* np = (ref_arena(nref) ? region : line) + ref_off(nref);
            bool same = true;
            for (int q = 0; q < s.c && same; ++q) same = np[q] == T.names[s.b + q];
            if (same) { cref = t[2 * k + 1]; found = true; }
        }
        if (found) setcookie_attr((ref_arena(cref) ? region : line) + ref_off(cref), ref_len(cref), s.a >> 8, v.kind, v.p, v.n, v.l);
        return v;
    }
    case TC_QP: {  // the parameter's last occurrence (ParsedRecord: the last value wins)
        const uint32_t cnt = C.q_count[s.a][i];
        if (cnt == 0) return v;
        const LP_G uint64_t* t = reinterpret_cast<const LP_G uint64_t*>(region + ref_off(C.q_params[s.a][i]));
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint64_t nref = t[2 * k];
            if (nref == REF_SKIP || ref_len(nref) != (uint32_t)s.c) continue;
            const LP_G uint8_t* np = (ref_arena(nref) ? region : line) + ref_off(nref);
            bool same = true;
            for (int q = 0; q < s.c && same; ++q) same = np[q] == T.names[s.b + q];
            if (same) ref(t[2 * k + 1]);
        }
        return v;
    }
    case TC_SCREEN: case TC_UNIQUEID: {  // the stage's source: a token, or the parameter's one occurrence
        const ValStage& S = P.val[s.a];
        const LP_G uint8_t* sp;
        uint32_t sn;
        if (S.src_tok >= 0) {
            if ((C.tok_flags[i] >> S.src_tok) & 1u) return v;  // "-": null, nothing is dissected
            const uint32_t w = C.tok_span[S.src_tok][i];
            sp = line + (w & 0xFFFFu);
            sn = (w >> 16) - (w & 0xFFFFu);
        } else {
            uint64_t vref = 0;
            if (qparam_source(P, S.src_q, S.src_qname, C, i, line, region, vref) != 1) return v;
            sp = (ref_arena(vref) ? region : line) + ref_off(vref);
            sn = ref_len(vref);
        }
        if (sn) remap_value(s.kind, s.b, sp, sn, v.kind, v.p, v.n, v.l, v.buf);
        return v;
    }
    default:  // TC_NONE, TC_NULL
        return v;
    }
}

// tvalue, or (GEO) a GeoIP output.  k_table_values has a GEO instance for
// tables with a TC_GEOIP source; its other instances compile to the code they
// were.  A GeoIP value is always a pointer word or a long of at most 62 bits
// (plan.cpp geo_field), never SW_SLOW: k_table_chars and the dictionary
// kernels, which derive only SW_SLOW values again, never meet one.  (As one more case of tvalue's switch, or as a test in front of
// it in the one instance, the GeoIP source changed the compiler's inlining and
// register allocation of k_table_values and k_dict_insert, which then ran 25 %
// to 100 % longer on columns that have nothing to do with it.)
// has_geo: some column of the table has such a source (host).
inline bool has_geo(const TableArgs& ta) {
    for (int c = 0; c < ta.n_cols; ++c)
        for (int f = 0; f < MAX_FMT; ++f)
            if (ta.cols[c].src[f].kind == TC_GEOIP || ta.cols[c].alt[f].kind == TC_GEOIP) return true;
    return false;
}
template <bool GEO>
__device__ __forceinline__ TVal tvalue_any(const Program& P, const Columns& C, const TableArgs& T, const TableSrc& s,
                                           int64_t i, const LP_G uint8_t* line, const LP_G uint8_t* region) {
    if constexpr (GEO) if (s.kind == TC_GEOIP) {
        TVal v;
        geo_value(C, P.val[s.a].want, s, i, v.kind, v.p, v.n, v.l);
        return v;
    }
    return tvalue(P, C, T, s, i, line, region);
}

// the row's line and arena region (a program without URI stages writes no
// region: nothing refers to one)
__device__ __forceinline__ bool row_view(const Program& P, const Columns& C, const uint8_t* buf, int64_t i,
                                         const LP_G uint8_t*& line, const LP_G uint8_t*& region) {
    if (C.status[i] != ST_OK) return false;
    line = (const LP_G uint8_t*)buf + C.line_off[i];
    region = P.has_phase2() ? C.arena + C.arena_base[i] : C.arena;
    return true;
}

// Row k's line of a row-list instance: rows[k] (null: first + k); false when
// it is outside the batch (never dereferenced: *bad_row is set, every lane
// that finds one stores the same 1)
__device__ __forceinline__ bool row_line(const LP_G int64_t* rows, int64_t first, int64_t n_lines, LP_G uint32_t* bad_row,
                                         int64_t k, int64_t& i) {
    i = rows ? rows[k] : first + k;
    if ((uint64_t)i < (uint64_t)n_lines) return true;
    *bad_row = 1u;
    return false;
}

}  // namespace

}  // namespace lp
