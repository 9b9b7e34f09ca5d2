// The term rules of lp_result_select_where (csrc/lp_pred.h) against plain C++:
// each byte op against memcmp / memmem / std::string, each LONG op against the
// operators, the outcome rule (null, NEGATE) and the group fold against their
// definitions in include/logparser_amd.h.  A program with its own main, built
// with -fsanitize=address,undefined (tests/test_select_where_sanitizers.py).
//
// Every value lives in a heap block of exactly its aligned-word extent: the
// block starts at a 4-byte boundary, the value at offset 0..3 in it, and the
// block ends with the aligned word that holds the value's last byte.  A read
// outside those words -- the bound lp_pred.h promises -- is an ASan error.
#ifndef _GNU_SOURCE
#define _GNU_SOURCE  // memmem
#endif
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../logparser_amd/csrc/lp_pred.h"

using namespace lp;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static long n_checks = 0;
static void fail(const char* what, int op, const std::string& v, const std::string& o, int view) {
    printf("FAIL %s op %d view %d value[%zu] operand[%zu]\n", what, op, view, v.size(), o.size());
    exit(1);
}

// the value's bytes at offset mis (0..3) of a block of exactly the aligned words that hold them
struct Block {
    uint8_t* base;
    uint8_t* p;
    Block(const std::string& v, unsigned mis) {
        const size_t ext = v.empty() ? 4 : (mis + v.size() + 3) & ~(size_t)3;
        base = (uint8_t*)aligned_alloc(4, ext);
        memset(base, 0xEE, ext);
        p = base + mis;
        if (!v.empty()) memcpy(p, v.data(), v.size());
    }
    ~Block() { free(base); }
};

static bool ref_bytes(int op, const std::string& v, const std::string& o) {
    switch (op) {
    case PRED_EQ: return v.size() == o.size() && memcmp(v.data(), o.data(), o.size()) == 0;
    case PRED_PREFIX: return v.size() >= o.size() && v.compare(0, o.size(), o) == 0;
    case PRED_SUFFIX: return v.size() >= o.size() && v.compare(v.size() - o.size(), o.size(), o) == 0;
    case PRED_CONTAINS: return o.empty() || memmem(v.data(), v.size(), o.data(), o.size()) != nullptr;
    default: return false;
    }
}

// one (value, operand): every byte op, plain and negated, null and not, through each view;
// amp: the value's first byte is the virtual '&' (v starts with it; the block holds the rest)
static void check_pair(const std::string& v, const std::string& o, bool amp) {
    static const int ops[] = {PRED_IS_NULL, PRED_EQ, PRED_PREFIX, PRED_SUFFIX, PRED_CONTAINS};
    const std::string stored = amp ? v.substr(1) : v;
    // the operand too in a block of its exact size: it is read byte by byte, [0, m)
    uint8_t* ob = (uint8_t*)malloc(o.size() ? o.size() : 1);
    if (!o.empty()) memcpy(ob, o.data(), o.size());
    for (unsigned mis = 0; mis < 4; ++mis) {
        Block B(stored, mis);
        for (int op : ops)
            for (int neg = 0; neg < 2; ++neg)
                for (int null = 0; null < 2; ++null) {
                    const int code = op | (neg ? PRED_NEGATE : 0);
                    const bool base = op == PRED_IS_NULL ? null != 0 : (!null && ref_bytes(op, v, o));
                    const bool want = base != (neg != 0);
                    PredBytes<const uint8_t*> vb{B.p, (uint32_t)stored.size(), amp};
                    PredWords<const uint8_t*, const uint32_t*> vw{B.p, (uint32_t)stored.size(), amp};
                    if (pred_term_bytes(code, null != 0, vb, (const uint8_t*)ob, (uint32_t)o.size()) != want)
                        fail("bytes", code, v, o, 0);
                    if (pred_term_bytes(code, null != 0, vw, (const uint8_t*)ob, (uint32_t)o.size()) != want)
                        fail("words", code, v, o, 1);
                    n_checks += 2;
                    if (!amp && v.size() <= 20 && mis == 0) {  // the local bytes of a formatted value
                        char* lb = (char*)malloc(v.size() ? v.size() : 1);
                        if (!v.empty()) memcpy(lb, v.data(), v.size());
                        PredLocal vl{lb, (uint32_t)v.size()};
                        if (pred_term_bytes(code, null != 0, vl, (const uint8_t*)ob, (uint32_t)o.size()) != want)
                            fail("local", code, v, o, 2);
                        free(lb);
                        ++n_checks;
                    }
                }
    }
    free(ob);
}

static std::string random_bytes(size_t n, int alphabet) {
    std::string s(n, '\0');
    for (auto& c : s) c = (char)(alphabet ? 'a' + rnd() % alphabet : rnd() & 0xFF);
    return s;
}

static void byte_ops() {
    const size_t lens[] = {0, 1, 3, 4, 5, 255};
    for (size_t vn : lens)
        for (size_t on : lens)
            for (int rep = 0; rep < 6; ++rep) {
                const int alphabet = rep < 2 ? 0 : rep < 4 ? 2 : 1;  // any byte; two letters (near misses); one letter
                std::string v = random_bytes(vn, alphabet);
                std::string o = random_bytes(on, alphabet);  // (an operand longer than the value among them)
                check_pair(v, o, false);
                if (on <= vn) {
                    check_pair(v, v.substr(0, on), false);        // a match at offset 0
                    check_pair(v, v.substr(vn - on), false);      // ... at the last possible offset
                    check_pair(v, v.substr((vn - on) / 2, on), false);
                    if (on > 0) {  // a near miss: the last byte differs
                        std::string m = v.substr(vn - on);
                        m[on - 1] = (char)(m[on - 1] ^ 1);
                        check_pair(v, m, false);
                    }
                }
                // the virtual leading '&': operands with and without it
                const std::string av = "&" + v;
                check_pair(av, o, true);
                check_pair(av, "&", true);
                check_pair(av, "&" + v.substr(0, on < vn ? on : vn), true);
                check_pair(av, av, true);
                if (on <= vn) check_pair(av, v.substr(vn - on), true);
            }
    // longer values: a needle whose first byte repeats
    for (int rep = 0; rep < 200; ++rep) {
        std::string v = random_bytes(1 + rnd() % 600, 2);
        std::string o = random_bytes(1 + rnd() % 6, 2);
        check_pair(v, o, false);
        check_pair("&" + v, o, true);
    }
}

static bool ref_long(int op, int64_t v, int64_t lo, int64_t hi) {
    switch (op) {
    case PRED_EQ: return v == lo;
    case PRED_LT: return v < lo;
    case PRED_LE: return v <= lo;
    case PRED_GT: return v > lo;
    case PRED_GE: return v >= lo;
    case PRED_BETWEEN: return !(v < lo) && !(hi < v);
    default: return false;
    }
}

static void long_ops() {
    std::vector<int64_t> xs = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, 499, 500, 599, 600, INT64_MAX - 1, INT64_MAX};
    for (int k = 0; k < 40; ++k) xs.push_back((int64_t)rnd());
    for (int op = PRED_IS_NULL; op <= PRED_BETWEEN; ++op)
        for (int neg = 0; neg < 2; ++neg)
            for (int null = 0; null < 2; ++null)
                for (int64_t v : xs)
                    for (int64_t lo : xs)
                        for (int64_t hi : {lo, INT64_MIN, INT64_MAX, (int64_t)600, (int64_t)-5}) {
                            const int code = op | (neg ? PRED_NEGATE : 0);
                            const bool base = op == PRED_IS_NULL ? null != 0 : (!null && ref_long(op, v, lo, hi));
                            if (pred_term_long(code, null != 0, v, lo, hi) != (base != (neg != 0))) {
                                printf("FAIL long op %d v %lld lo %lld hi %lld\n", code, (long long)v, (long long)lo, (long long)hi);
                                exit(1);
                            }
                            ++n_checks;
                        }
}

static void op_table() {
    for (int op = -2; op < 14; ++op)
        for (int neg = 0; neg < 2; ++neg) {
            const int code = op | (neg ? PRED_NEGATE : 0);
            const bool s = op == 0 || op == 1 || (op >= 7 && op <= 9), l = op >= 0 && op <= 6;
            if (op >= 0 && (pred_op_ok(code, 1) != s || pred_op_ok(code, 2) != l)) { printf("FAIL op table %d\n", code); exit(1); }
            if (op < 0 && (pred_op_ok(op, 1) || pred_op_ok(op, 2))) { printf("FAIL op table %d\n", op); exit(1); }
            ++n_checks;
        }
    if (pred_op_ok(PRED_EQ | 0x200, 1) || pred_op_ok(PRED_EQ, 4)) { printf("FAIL op table bits\n"); exit(1); }
}

// the fold against its definition: AND over the groups of OR over the group's terms
static void fold() {
    for (int n = 0; n <= PRED_MAX_TERMS; ++n)
        for (int rep = 0; rep < 400; ++rep) {
            int group[PRED_MAX_TERMS], out[PRED_MAX_TERMS], g = (int)(rnd() % 3);
            for (int t = 0; t < n; ++t) {
                if (t && rnd() % 2) g += 1 + (int)(rnd() % 2);
                group[t] = g;
                out[t] = (int)(rnd() % 2);
            }
            bool want = true;
            for (int t = 0; t < n;) {
                bool any = false;
                int e = t;
                for (; e < n && group[e] == group[t]; ++e) any = any || out[e];
                want = want && any;
                t = e;
            }
            PredFold F;
            int evaluated = 0;
            for (int t = 0; t < n; ++t) {
                pred_fold_group(F, t, group[t]);
                if (!pred_fold_wants(F)) continue;  // (a decided line evaluates no further term)
                pred_fold_term(F, out[t] != 0);
                ++evaluated;
            }
            if (pred_fold_result(F, n) != want || evaluated > n) { printf("FAIL fold n %d\n", n); exit(1); }
            ++n_checks;
        }
}

int main() {
    op_table();
    long_ops();
    byte_ops();
    fold();
    printf("ok %ld\n", n_checks);
    return 0;
}
