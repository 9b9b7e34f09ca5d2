// TEST-ONLY: the owner lookup of the URI kernels' cooperative passes
// (logparser_amd/csrc/lp_owner.h) on the CPU.  For a vector of per-lane item
// counts, the exclusive prefix, the mask N of non-empty lanes and per round
// of 64 items K and the head mask H are computed the way uri.hip's
// OwnerRounds computes them; for every item g the helper's owner must equal
// the definition, "the last lane whose first item is <= g", found by a
// linear scan, and the rank table the kernel reads (entry r: the r-th
// non-empty lane and its first item, written by that lane at the count of
// non-empty lanes below it) must give the same lane and its first item.
//
// Built as a ctypes library (tests/owner_emu_lib.py) and, with -DOW_MAIN, as
// a stand-alone program that runs every group (for a sanitizer build).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../logparser_amd/csrc/lp_owner.h"

namespace {

constexpr int PW = 64;
typedef std::vector<uint32_t> Counts;  // PW per-lane counts

struct Result {
    int64_t vectors = 0, items = 0, rounds = 0, empty_rounds = 0, differ = 0;
    std::string first;  // the first difference
};

void differ(Result& R, const Counts& c, uint32_t g, const char* what, long got, long want) {
    if (R.differ++ == 0) {
        char b[256];
        snprintf(b, sizeof b, "item %u: %s %ld, expected %ld; counts", g, what, got, want);
        R.first = b;
        for (int l = 0; l < PW; ++l) R.first += " " + std::to_string(c[l]);
    }
}

void check(const Counts& c, Result& R) {
    uint32_t first[PW], total = 0;
    uint64_t N = 0;
    for (int l = 0; l < PW; ++l) {
        first[l] = total;
        total += c[l];
        if (c[l]) N |= 1ull << l;
    }
    uint32_t tab[PW] = {};  // as OwnerRounds' constructor fills it
    for (int l = 0; l < PW; ++l)
        if (c[l]) tab[__builtin_popcountll(N & ((1ull << l) - 1ull))] = (uint32_t)l | first[l] << 6;
    ++R.vectors;
    for (uint32_t g0 = 0; g0 < total; g0 += PW) {
        // the round's K and head mask, as OwnerRounds::fill / owner
        uint64_t before = 0, H = 0;
        for (int l = 0; l < PW; ++l) {
            if (c[l] && first[l] < g0) before |= 1ull << l;
            if (c[l] && first[l] >= g0 && ((first[l] - g0) >> 6) == 0) H |= 1ull << (first[l] & 63u);
        }
        const uint32_t K = (uint32_t)__builtin_popcountll(before);
        ++R.rounds;
        if (!H) ++R.empty_rounds;
        for (int i = 0; i < PW; ++i) {
            const uint32_t g = g0 + (uint32_t)i;
            const int ow = lp::owner_lane(N, K, H, i);
            const uint32_t rank = lp::owner_rank(K, H, i);
            const uint32_t e = tab[(rank - 1u) & 63u];
            int want = 0;  // the definition: the last lane whose first item is <= g
            for (int l = 0; l < PW; ++l)
                if (first[l] <= g) want = l;
            if (g >= total) {  // no such item: the last non-empty lane, in range for a shuffle
                want = 63 - __builtin_clzll(N);
            } else {
                ++R.items;
                if (!(c[want] && first[want] <= g && g < first[want] + c[want])) differ(R, c, g, "definition", want, -1);
            }
            if (ow != want) differ(R, c, g, "owner", ow, want);
            if (rank < 1 || rank > (uint32_t)__builtin_popcountll(N)) differ(R, c, g, "rank", (long)rank, -1);
            if ((int)(e & 63u) != want) differ(R, c, g, "table lane", (long)(e & 63u), want);
            if (e >> 6 != first[want]) differ(R, c, g, "table first item", (long)(e >> 6), (long)first[want]);
        }
    }
    // select64 on its own: the k-th set bit of N
    for (uint32_t k = 0, l = 0; l < PW; ++l)
        if ((N >> l) & 1) {
            if (lp::select64(N, k) != l) differ(R, c, k, "select64", (long)lp::select64(N, k), (long)l);
            ++k;
        }
}

Counts zeros() { return Counts(PW, 0u); }

const char* const GROUPS[] = {"all-ones", "single-lane", "lane-pairs", "empty-runs", "totals", "random"};
constexpr int N_GROUPS = 6;

Result run_group(int gi) {
    Result R;
    switch (gi) {
    case 0: {
        check(Counts(PW, 1u), R);
        break;
    }
    case 1:
        for (int lane : {0, 31, 63})
            for (uint32_t n : {1u, 63u, 64u, 65u, 129u, 600u}) {
                Counts c = zeros();
                c[lane] = n;
                check(c, R);
            }
        break;
    case 2:
        for (int lane : {0, 31, 62})
            for (uint32_t x : {0u, 1u, 63u, 64u, 65u})
                for (uint32_t y : {0u, 1u, 63u, 64u, 65u}) {
                    Counts c = zeros();
                    c[lane] = x;
                    c[lane + 1] = y;
                    check(c, R);
                }
        break;
    case 3:
        // `run` empty lanes directly before the lane whose first item is T;
        // the T items before them in one lane or in two
        for (uint32_t T : {64u, 128u})
            for (int run : {1, 2, 40})
                for (int split = 0; split < 2; ++split)
                    for (uint32_t own : {1u, 64u, 65u}) {
                        Counts c = zeros();
                        int l = 0;
                        if (split) {
                            c[l++] = T - 1;
                            c[l++] = 1;
                        } else {
                            c[l++] = T;
                        }
                        l += run;
                        c[l++] = own;
                        c[l] = 1;
                        c[63] = 2;
                        check(c, R);
                    }
        break;
    case 4:
        for (uint32_t t : {0u, 1u, 63u, 64u, 65u, 127u, 128u, 129u}) {
            Counts c = zeros();  // spread over the lanes from lane 0
            for (int l = 0; l < PW; ++l) c[l] = t / PW + ((uint32_t)l < t % PW ? 1u : 0u);
            check(c, R);
            c = zeros();  // from lane 63 down
            for (int l = 0; l < PW; ++l) c[63 - l] = t / PW + ((uint32_t)l < t % PW ? 1u : 0u);
            check(c, R);
            c = zeros();  // in one lane
            c[17] = t;
            check(c, R);
            c = zeros();  // in two lanes far apart
            c[5] = t / 2;
            c[50] = t - t / 2;
            check(c, R);
        }
        break;
    case 5: {
        static const uint32_t pick[9] = {0, 0, 0, 1, 2, 5, 17, 64, 130};
        uint64_t s = 0x9E3779B97F4A7C15ull;  // the seed (xorshift64*)
        for (int v = 0; v < 20000; ++v) {
            Counts c = zeros();
            for (int l = 0; l < PW; ++l) {
                s ^= s >> 12;
                s ^= s << 25;
                s ^= s >> 27;
                c[l] = pick[((s * 0x2545F4914F6CDD1Dull) >> 33) % 9];
            }
            check(c, R);
        }
        break;
    }
    }
    return R;
}

}  // namespace

extern "C" {
int ow_groups() { return N_GROUPS; }
const char* ow_group_name(int gi) { return gi >= 0 && gi < N_GROUPS ? GROUPS[gi] : ""; }
// runs group gi: stats = {vectors, items, rounds, rounds without a head}; returns the differences
int64_t ow_run_group(int gi, int64_t* stats, char* first, int cap) {
    const Result R = run_group(gi);
    stats[0] = R.vectors;
    stats[1] = R.items;
    stats[2] = R.rounds;
    stats[3] = R.empty_rounds;
    if (cap > 0) snprintf(first, (size_t)cap, "%s", R.first.c_str());
    return R.differ;
}
// one vector of 64 counts given by the caller
int64_t ow_check(const uint32_t* counts, int64_t* items, char* first, int cap) {
    Result R;
    check(Counts(counts, counts + PW), R);
    *items = R.items;
    if (cap > 0) snprintf(first, (size_t)cap, "%s", R.first.c_str());
    return R.differ;
}
}

#ifdef OW_MAIN
int main() {
    int64_t bad = 0;
    for (int gi = 0; gi < N_GROUPS; ++gi) {
        const Result R = run_group(gi);
        printf("%s: %lld vectors, %lld items, %lld rounds (%lld without a head), %lld differ%s%s\n", GROUPS[gi],
               (long long)R.vectors, (long long)R.items, (long long)R.rounds, (long long)R.empty_rounds,
               (long long)R.differ, R.differ ? ": " : "", R.first.c_str());
        bad += R.differ;
    }
    return bad ? 1 : 0;
}
#endif
