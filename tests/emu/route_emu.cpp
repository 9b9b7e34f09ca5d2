// TEST-ONLY: the transition-table algebra of the sticky routing scan
// (fmt_table, fmt_compose, fmt_apply, lp_device.h) on the CPU, against a plain
// loop that restates HttpdLogFormatDissector.dissect one line at a time, and
// the scan's shape (kernels.hip: 64 lines per lane, a 64-lane inclusive scan
// in doubling order, one serial pass over the chunks) against the serial
// fold.  A stand-alone program: it prints what it checked and exits 0, or
// prints the first differences and exits 1.  Built under ASan + UBSan by
// tests/test_sticky_routing.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../logparser_amd/csrc/lp_device.h"

namespace {

using lp::FMT_UNKNOWN;

constexpr uint64_t IDENTITY = 0xFEDCBA9876543210ull;
constexpr int LANES = 64, LINES_PER_LANE = 64, CHUNK_LINES = LANES * LINES_PER_LANE;

// The Java rule from a known state s < nf (m: bit f = format f matches, bit
// 8 + f = format f is not decided): the active format when it matches; else
// the formats in order, the first that matches; when none matches the state
// stays.  Wherever the answer would need an undecided format's result, the
// state is unknown.
uint32_t rule_known(uint32_t m, int nf, uint32_t s) {
    const auto yes = [&](int f) { return (m >> f) & 1u; };
    const auto maybe = [&](int f) { return !yes(f) && ((m >> (8 + f)) & 1u); };
    if (yes((int)s)) return s;
    if (maybe((int)s)) return FMT_UNKNOWN;
    for (int f = 0; f < nf; ++f) {
        if (yes(f)) return (uint32_t)f;
        if (maybe(f)) return FMT_UNKNOWN;
    }
    return s;
}

// ... and from any state: an unknown state becomes known only when every
// known state leads to the same format; the states nf..14 do not occur
uint32_t rule(uint32_t m, int nf, uint32_t s) {
    if (s < (uint32_t)nf) return rule_known(m, nf, s);
    if (s != FMT_UNKNOWN) return FMT_UNKNOWN;
    const uint32_t r = rule_known(m, nf, 0);
    for (int x = 1; x < nf; ++x)
        if (rule_known(m, nf, (uint32_t)x) != r) return FMT_UNKNOWN;
    return r;
}

long g_checked = 0;
int g_failed = 0;

void expect(bool ok, const char* what, uint64_t a, uint64_t b, uint64_t c) {
    ++g_checked;
    if (!ok && g_failed++ < 10)
        std::printf("DIFF (%s): %016llx %016llx %016llx\n", what, (unsigned long long)a, (unsigned long long)b,
                    (unsigned long long)c);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// a match word as the kernels produce them: usually decided (one format, two,
// none), sometimes with undecided bits, sometimes every undecided bit
uint32_t random_word(int nf) {
    const uint32_t all = (1u << nf) - 1u;
    const uint32_t r = rnd();
    uint32_t c = 0;
    switch (r & 3u) {
    case 0: c = 1u << (rnd() % (uint32_t)nf); break;
    case 1: c = (1u << (rnd() % (uint32_t)nf)) | (1u << (rnd() % (uint32_t)nf)); break;
    case 2: c = 0; break;
    default: c = rnd() & all; break;
    }
    uint32_t u = 0;
    if ((r >> 2) % 50 == 0) u = all;
    else if ((r >> 2) % 50 == 1) u = rnd() & all;
    if (u == all) c = 0;
    return c | ((u & ~c) << 8);
}

uint64_t random_table(int nf) {
    uint64_t t = IDENTITY;
    for (int k = rnd() % 4; k >= 0; --k) t = lp::fmt_compose(t, lp::fmt_table(random_word(nf), nf));
    return t;
}

// the states of the lines of `words` as the three routing kernels compute
// them: per chunk of 4096 lines the lanes' tables and their inclusive scan
// (k_fmt_reduce), the chunks' entry states (k_fmt_chunks), then each lane from
// the exclusive prefix (k_fmt_apply)
std::vector<uint32_t> scan_states(const std::vector<uint32_t>& words, int nf, uint32_t init, uint32_t* final_state) {
    const int64_t n = (int64_t)words.size();
    const int64_t n_chunks = (n + CHUNK_LINES - 1) / CHUNK_LINES;
    std::vector<uint64_t> incl((size_t)(n_chunks * LANES));
    for (int64_t c = 0; c < n_chunks; ++c) {
        uint64_t t[LANES];
        for (int lane = 0; lane < LANES; ++lane) {
            t[lane] = IDENTITY;
            for (int k = 0; k < LINES_PER_LANE; ++k) {
                const int64_t li = c * CHUNK_LINES + (int64_t)lane * LINES_PER_LANE + k;
                if (li >= n) break;
                t[lane] = lp::fmt_compose(t[lane], lp::fmt_table(words[(size_t)li], nf));
            }
        }
        for (int d = 1; d < LANES; d <<= 1) {  // every lane reads its neighbour's value of the round before
            uint64_t o[LANES];
            for (int lane = 0; lane < LANES; ++lane) o[lane] = lane >= d ? t[lane - d] : 0;
            for (int lane = d; lane < LANES; ++lane) t[lane] = lp::fmt_compose(o[lane], t[lane]);
        }
        for (int lane = 0; lane < LANES; ++lane) incl[(size_t)(c * LANES + lane)] = t[lane];
    }
    std::vector<uint32_t> entry((size_t)n_chunks + 1);
    uint32_t s = init;
    for (int64_t c = 0; c < n_chunks; ++c) {
        entry[(size_t)c] = s;
        s = lp::fmt_apply(incl[(size_t)(c * LANES + LANES - 1)], s);
    }
    *final_state = s;
    std::vector<uint32_t> out((size_t)n);
    for (int64_t c = 0; c < n_chunks; ++c)
        for (int lane = 0; lane < LANES; ++lane) {
            const uint64_t excl = lane ? incl[(size_t)(c * LANES + lane - 1)] : IDENTITY;
            uint32_t st = lp::fmt_apply(excl, entry[(size_t)c]);
            for (int k = 0; k < LINES_PER_LANE; ++k) {
                const int64_t li = c * CHUNK_LINES + (int64_t)lane * LINES_PER_LANE + k;
                if (li >= n) break;
                st = lp::fmt_apply(lp::fmt_table(words[(size_t)li], nf), st);
                out[(size_t)li] = st;
            }
        }
    return out;
}

}  // namespace

int main(int argc, char** argv) {
    const long n_random = argc > 1 ? std::atol(argv[1]) : 20000;
    // 1. every table against the rule: every nf, every 16-bit word, every state
    for (int nf = 1; nf <= 8; ++nf)
        for (uint32_t m = 0; m < 65536; ++m) {
            const uint64_t t = lp::fmt_table(m, nf);
            for (uint32_t s = 0; s < 16; ++s)
                expect(lp::fmt_apply(t, s) == rule(m, nf, s), "fmt_table", ((uint64_t)nf << 32) | m, s, t);
        }
    const long n_tables = g_checked;
    // 2. the identity, composition against application, associativity
    for (long k = 0; k < n_random; ++k) {
        const int nf = 1 + (int)(rnd() % 8);
        const uint64_t a = random_table(nf), b = random_table(nf), c = random_table(nf);
        expect(lp::fmt_compose(IDENTITY, a) == a, "identity o t", a, 0, 0);
        expect(lp::fmt_compose(a, IDENTITY) == a, "t o identity", a, 0, 0);
        const uint64_t ab = lp::fmt_compose(a, b);
        for (uint32_t s = 0; s < 16; ++s)
            expect(lp::fmt_apply(ab, s) == lp::fmt_apply(b, lp::fmt_apply(a, s)), "compose / apply", a, b, s);
        expect(lp::fmt_compose(ab, c) == lp::fmt_compose(a, lp::fmt_compose(b, c)), "associativity", a, b, c);
    }
    // 3. sequences of words: the composed table of a prefix applied to the
    // initial state = the rule, line after line
    for (long k = 0; k < n_random / 20; ++k) {
        const int nf = 1 + (int)(rnd() % 8);
        const uint32_t init = rnd() % 5 == 0 ? FMT_UNKNOWN : rnd() % (uint32_t)nf;
        uint64_t t = IDENTITY;
        uint32_t s = init;
        for (int i = 0; i < 200; ++i) {
            const uint32_t m = random_word(nf);
            t = lp::fmt_compose(t, lp::fmt_table(m, nf));
            s = rule(m, nf, s);
            expect(lp::fmt_apply(t, init) == s, "prefix table", m, init, t);
        }
    }
    // 4. the scan's tree against the serial fold: whole chunks, a partial last
    // lane and chunk, one line, and lengths around the lane and chunk sizes
    const int64_t lengths[] = {1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 3 * 4096 + 1000};
    long n_lines = 0;
    for (int64_t n : lengths)
        for (int rep = 0; rep < 6; ++rep) {
            const int nf = rep < 2 ? 4 : 1 + (int)(rnd() % 8);
            const uint32_t init = rep == 1 ? FMT_UNKNOWN : rnd() % (uint32_t)nf;
            std::vector<uint32_t> words((size_t)n);
            for (auto& w : words) w = random_word(nf);
            if (rep == 0)  // long runs that only compose: two formats match every line but a few
                for (auto& w : words) w = rnd() % 300 ? 3u : w;
            uint32_t fin = 0;
            const std::vector<uint32_t> got = scan_states(words, nf, init, &fin);
            uint32_t s = init;
            for (int64_t i = 0; i < n; ++i) {
                s = rule(words[(size_t)i], nf, s);
                expect(got[(size_t)i] == s, "scan state", (uint64_t)i, got[(size_t)i], s);
            }
            expect(fin == s, "scan final state", (uint64_t)n, fin, s);
            n_lines += n;
        }
    std::printf("route_emu: %ld table entries, %ld random tables, %ld scanned lines, %ld checks, %d differ\n", n_tables,
                n_random, n_lines, g_checked, g_failed);
    return g_failed ? 1 : 0;
}
