// TEST-ONLY stand-alone program (its own main): the core of the grouped
// aggregates (logparser_amd/csrc/lp_group.h over lp_dict.h) on the CPU, built
// with ASan + UBSan (and ThreadSanitizer) and run directly by
// tests/test_group_by_sanitizers.py.  Rows of two keys (a STRING or null, a
// LONG or null) and two measures go through
//   - the key tuple's hash and lp_dict.h's insert with lp_group.h's same(r)
//     rule (the stored hash first -- 0 while it is not seen --, then the keys
//     in full), from 1, 4 and 7 std::threads, the hash whole and narrowed to 1 bit;
//   - the accumulation in the privatised shape (each thread a "block": a local
//     copy at the identities, its rows folded in, the touched words flushed
//     with one atomic each) and in the direct shape (64-row "waves" whose
//     leading groups are merged for a fixed number of rounds, one atomic per
//     word, the rows left folding on their own);
// and every run must give the groups, their numbering by first occurrence and
// the aggregates' value / valid of a std::map built in row order.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../logparser_amd/csrc/lp_group.h"

namespace {

struct Row {
    bool s_null, l_null;
    std::string s;
    int64_t l;
    bool m_ok[2];
    int64_t m[2];
};

std::vector<Row> corpus() {
    std::vector<Row> v;
    const char* strs[] = {"", "a", "ab", "abcdefgh", "abcdefghi", "abcdefgX", "GET", "GET", "GET", "GET", "POST"};
    for (int k = 0; k < 3000; ++k) {
        Row r{};
        r.s_null = k % 13 == 5;
        r.s = r.s_null ? "" : k % 10 == 9 ? "only-" + std::to_string(k) : strs[k * 7 % 11];
        r.l_null = k % 17 == 3;
        r.l = r.l_null ? 0 : k % 4 == 0 ? 200 : (int64_t)(k % 5) - 2;
        r.m_ok[0] = k % 6 != 1;
        r.m[0] = k % 50 == 0 ? INT64_MAX : k % 50 == 1 ? INT64_MIN : (int64_t)k * 1000003 - 1500000000;
        r.m_ok[1] = r.s == "POST" ? false : k % 3 == 0;  // a group whose measure is null on every row
        r.m[1] = -(int64_t)k;
        v.push_back(r);
    }
    return v;
}

uint64_t hash_of(const Row& r, int bits) {
    uint64_t h = lp::GROUP_SEED;
    if (r.s_null) h = lp::group_hash_null(h);
    else
        h = lp::group_hash_bytes(h, (uint32_t)r.s.size(), [&](uint32_t j) {
            uint64_t w = 0;
            const size_t o = 8 * (size_t)j;
            memcpy(&w, r.s.data() + o, r.s.size() - o < 8 ? r.s.size() - o : 8);
            return w;
        });
    h = r.l_null ? lp::group_hash_null(h) : lp::group_hash_long(h, r.l);
    return lp::group_hash_end(h, bits);
}

bool keys_equal(const Row& a, const Row& b) {
    if (a.s_null != b.s_null || a.l_null != b.l_null) return false;
    return (a.s_null || a.s == b.s) && (a.l_null || a.l == b.l);
}

typedef std::tuple<bool, std::string, bool, int64_t> Key;
Key key_of(const Row& r) { return Key(r.s_null, r.s_null ? "" : r.s, r.l_null, r.l_null ? 0 : r.l); }

int differ = 0;
void expect(bool ok, const char* what, long a = 0, long b = 0) {
    if (ok) return;
    if (++differ < 20) printf("DIFFER %s (%ld, %ld)\n", what, a, b);
}

// the groups of the rows, numbered by first occurrence, through the hash table
std::vector<int32_t> group_rows(const std::vector<Row>& v, int threads, int bits, std::vector<int64_t>& reps) {
    const uint32_t n = (uint32_t)v.size(), cap = lp::dict_capacity(n);
    std::vector<uint32_t> slots(cap, lp::DICT_EMPTY), slot(n, lp::DICT_EMPTY);
    std::vector<uint64_t> hash(n, 0);  // zeroed: not seen
    auto work = [&](uint32_t a, uint32_t step) {
        for (uint32_t k = a; k < n; k += step) {
            const uint64_t h = hash_of(v[k], bits);
            lp::GroupAtHost::store_hash(&hash[k], h);
            auto same = [&](uint32_t r) {
                if (!lp::group_hash_may_equal(lp::GroupAtHost::load_hash(&hash[r]), h)) return false;
                return keys_equal(v[k], v[r]);
            };
            slot[k] = lp::dict_insert<lp::DictAtHost>(slots.data(), cap, lp::dict_home(h, cap, bits), k, same);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work, (uint32_t)t, (uint32_t)threads);
    work(0, (uint32_t)threads);
    for (auto& th : pool) th.join();
    // mark / rank / index, as dict.hip
    std::vector<uint32_t> rank(n, 0);
    uint32_t run = 0;
    for (uint32_t k = 0; k < n; ++k) {
        expect(slot[k] != lp::DICT_EMPTY, "a probe ran out", k);
        if (slot[k] != lp::DICT_EMPTY && slots[slot[k]] == k) {
            ++run;
            reps.push_back(k);
        }
        rank[k] = run;
    }
    std::vector<int32_t> group_of(n, 0);
    for (uint32_t k = 0; k < n; ++k)
        if (slot[k] != lp::DICT_EMPTY) group_of[k] = (int32_t)(rank[slots[slot[k]]] - 1);
    return group_of;
}

struct Local {  // a block's own copy / a wave's partial: no atomics
    static void fetch_add(int64_t* p, int64_t v) { *p = (int64_t)((uint64_t)*p + (uint64_t)v); }
    static void fetch_min(int64_t* p, int64_t v) { if (v < *p) *p = v; }
    static void fetch_max(int64_t* p, int64_t v) { if (v > *p) *p = v; }
};

int64_t contrib(const lp::GroupAccs& A, const Row& r, int w) {
    const int m = A.wmeas[w];
    return lp::group_contrib(A.wkind[w], m >= 0 && r.m_ok[m], m >= 0 ? r.m[m] : 0);
}

std::vector<int64_t> accumulate(const std::vector<Row>& v, const std::vector<int32_t>& group_of, size_t n_groups,
                                const lp::GroupAccs& A, int threads, bool privatised, int peel) {
    const int W = A.n_words;
    std::vector<int64_t> acc(n_groups * W);
    for (size_t x = 0; x < acc.size(); ++x) acc[x] = lp::group_identity(A.wkind[x % W]);
    auto work = [&](size_t t) {
        if (privatised) {  // block t: rows t*64.. in strides, as the kernel's grid-stride loop
            std::vector<int64_t> loc(acc.size());
            for (size_t x = 0; x < loc.size(); ++x) loc[x] = lp::group_identity(A.wkind[x % W]);
            for (size_t k0 = t * 64; k0 < v.size(); k0 += (size_t)threads * 64)
                for (size_t k = k0; k < k0 + 64 && k < v.size(); ++k)
                    for (int w = 0; w < W; ++w)
                        lp::group_fold<Local>(&loc[(size_t)group_of[k] * W + w], A.wkind[w], contrib(A, v[k], w));
            for (size_t x = 0; x < loc.size(); ++x) lp::group_fold<lp::GroupAtHost>(&acc[x], A.wkind[x % W], loc[x]);
            return;
        }
        for (size_t k0 = t * 64; k0 < v.size(); k0 += (size_t)threads * 64) {  // one wave of 64 rows
            const size_t k1 = k0 + 64 < v.size() ? k0 + 64 : v.size();
            std::vector<char> cand(k1 - k0, 1), mine(k1 - k0, 1);
            for (int round = 0; round < peel; ++round) {
                size_t lead = k0;
                while (lead < k1 && !cand[lead - k0]) ++lead;
                if (lead == k1) break;
                const int32_t g = group_of[lead];
                size_t share = 0;
                for (size_t k = lead; k < k1; ++k) share += cand[k - k0] && group_of[k] == g;
                std::vector<int64_t> part(W);
                for (int w = 0; w < W; ++w) part[w] = lp::group_identity(A.wkind[w]);
                for (size_t k = lead; k < k1; ++k) {
                    if (!cand[k - k0] || group_of[k] != g) continue;
                    cand[k - k0] = 0;
                    if (share < 2) continue;
                    mine[k - k0] = 0;
                    for (int w = 0; w < W; ++w) part[w] = lp::group_merge(A.wkind[w], part[w], contrib(A, v[k], w));
                }
                if (share >= 2)
                    for (int w = 0; w < W; ++w) lp::group_fold<lp::GroupAtHost>(&acc[(size_t)g * W + w], A.wkind[w], part[w]);
            }
            for (size_t k = k0; k < k1; ++k)
                if (mine[k - k0])
                    for (int w = 0; w < W; ++w)
                        lp::group_fold<lp::GroupAtHost>(&acc[(size_t)group_of[k] * W + w], A.wkind[w], contrib(A, v[k], w));
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(work, (size_t)t);
    work(0);
    for (auto& th : pool) th.join();
    return acc;
}

}  // namespace

int main() {
    const std::vector<Row> v = corpus();
    // the reference: a std::map in row order
    std::map<Key, int32_t> seen;
    std::vector<int32_t> want_group;
    std::vector<int64_t> want_reps;
    for (size_t k = 0; k < v.size(); ++k) {
        auto it = seen.find(key_of(v[k]));
        if (it == seen.end()) {
            it = seen.emplace(key_of(v[k]), (int32_t)want_reps.size()).first;
            want_reps.push_back((int64_t)k);
        }
        want_group.push_back(it->second);
    }
    const size_t G = want_reps.size();
    const int32_t ops[8] = {lp::GA_COUNT_ROWS, lp::GA_SUM, lp::GA_MIN, lp::GA_MAX, lp::GA_COUNT, lp::GA_SUM, lp::GA_COUNT, lp::GA_MAX};
    const int32_t meas[8] = {-1, 0, 0, 0, 0, 1, 1, 1};
    const lp::GroupAccs A = lp::group_accs(8, ops, meas, 2);
    expect(A.n_words == 1 + 2 + 5, "accumulator words", A.n_words);
    // ... and its aggregates, with unsigned (wrapping) sums
    std::vector<std::vector<int64_t>> want_val(8, std::vector<int64_t>(G, 0));
    std::vector<std::vector<uint8_t>> want_ok(8, std::vector<uint8_t>(G, 0));
    for (int a = 0; a < 8; ++a) {
        std::vector<uint64_t> n(G, 0), sum(G, 0);
        std::vector<int64_t> lo(G, INT64_MAX), hi(G, INT64_MIN);
        for (size_t k = 0; k < v.size(); ++k) {
            const size_t g = (size_t)want_group[k];
            if (ops[a] == lp::GA_COUNT_ROWS) { ++n[g]; continue; }
            if (!v[k].m_ok[meas[a]]) continue;
            const int64_t x = v[k].m[meas[a]];
            ++n[g];
            sum[g] += (uint64_t)x;
            if (x < lo[g]) lo[g] = x;
            if (x > hi[g]) hi[g] = x;
        }
        for (size_t g = 0; g < G; ++g) {
            want_ok[a][g] = ops[a] <= lp::GA_COUNT || n[g] > 0;
            if (!want_ok[a][g]) continue;
            want_val[a][g] = ops[a] <= lp::GA_COUNT ? (int64_t)n[g] : ops[a] == lp::GA_SUM ? (int64_t)sum[g]
                             : ops[a] == lp::GA_MIN ? lo[g] : hi[g];
        }
    }
    bool some_invalid = false;
    for (size_t g = 0; g < G; ++g) some_invalid = some_invalid || !want_ok[5][g];
    expect(some_invalid, "the corpus has a group without a value");
    for (int bits : {0, 1})
        for (int threads : {1, 4, 7}) {
            std::vector<int64_t> reps;
            const std::vector<int32_t> group_of = group_rows(v, threads, bits, reps);
            expect(reps == want_reps, "representatives", (long)reps.size(), (long)G);
            expect(group_of == want_group, "group_of");
            if (reps != want_reps || group_of != want_group) continue;
            for (int shape = 0; shape < 3; ++shape) {  // privatised; direct with 2 peel rounds; direct without
                const std::vector<int64_t> acc = accumulate(v, group_of, G, A, threads, shape == 0, shape == 1 ? 2 : 0);
                for (size_t g = 0; g < G; ++g)
                    for (int a = 0; a < 8; ++a) {
                        uint8_t ok = 0;
                        const int64_t x = lp::group_value(A, a, &acc[g * A.n_words], ok);
                        expect(ok == want_ok[a][g] && x == want_val[a][g], "aggregate", (long)g, a);
                    }
            }
            printf("bits %d threads %d: %zu groups\n", bits, threads, G);
        }
    // the regime's boundary: the need against the budget
    const int64_t need = (int64_t)G * A.n_words;
    expect(lp::group_privatised((int64_t)G, A.n_words, need) && lp::group_privatised((int64_t)G, A.n_words, need + 1) &&
               !lp::group_privatised((int64_t)G, A.n_words, need - 1) && !lp::group_privatised(1, 1, 0),
           "regime boundary");
    // the fold's identities are never issued, the merge wraps
    expect(lp::group_merge(lp::GA_SUM, INT64_MAX, INT64_MAX) == -2 && lp::group_merge(lp::GA_MIN, INT64_MAX, 3) == 3 &&
               lp::group_merge(lp::GA_MAX, INT64_MIN, -3) == -3,
           "merge");
    printf("total: %d differ\n", differ);
    return differ ? 1 : 0;
}
