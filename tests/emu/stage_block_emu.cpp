// TEST-ONLY: the 64-byte block core of the chunk kernel's staging pass
// (bcls::classify64p, lp_device.h) on the CPU, against build_masks and a
// byte-by-byte restatement of what its outputs mean.  A stand-alone program:
// it prints the number of blocks checked and exits 0, or prints the first
// differences and exits 1.  Built plain and under ASan + UBSan by
// tests/test_stage_block.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../logparser_amd/csrc/lp_device.h"

namespace {

struct Ref {
    uint64_t p0, p1, lf;
    uint32_t g[4], other;
};

// what the outputs mean, byte by byte (no SWAR): byte i of the block -> bit i
// of a plane word; byte 4 k + c of piece j -> bit 8 c + 7 of g[j] / other
Ref reference(const uint8_t* b) {
    Ref r{};
    for (int i = 0; i < 64; ++i) {
        const uint8_t c = b[i];
        const int j = i >> 4, col = i & 3;
        if (c == '"') r.p0 |= 1ull << i;
        if (c <= 0x20) r.p1 |= 1ull << i;
        if (c == '\n') r.lf |= 1ull << i;
        if (c >= 0x7F) r.g[j] |= 0x80u << (8 * col);
        if (c < 0x20 && c != '\n') r.other |= 0x80u << (8 * col);
    }
    return r;
}

long g_checked = 0;
int g_failed = 0;

void check(const uint8_t* b, const char* what) {
    uint32_t w[16];
    std::memcpy(w, b, 64);
    const lp::bcls::Block64 K = lp::bcls::classify64p(w);
    const Ref r = reference(b);
    uint64_t m[2];
    lp::build_masks(b, 64, m);
    bool ok = K.p0 == r.p0 && K.p1 == r.p1 && K.lf == r.lf && K.other == r.other && K.p0 == m[0] && K.p1 == m[1];
    for (int j = 0; j < 4; ++j) ok = ok && K.g[j] == r.g[j];
    ++g_checked;
    if (!ok && g_failed++ < 5) {
        std::printf("DIFF (%s):", what);
        for (int i = 0; i < 64; ++i) std::printf(" %02x", b[i]);
        std::printf("\n  core p0 %016llx p1 %016llx lf %016llx g %08x %08x %08x %08x other %08x\n",
                    (unsigned long long)K.p0, (unsigned long long)K.p1, (unsigned long long)K.lf, K.g[0], K.g[1],
                    K.g[2], K.g[3], K.other);
        std::printf("  ref  p0 %016llx p1 %016llx lf %016llx g %08x %08x %08x %08x other %08x\n",
                    (unsigned long long)r.p0, (unsigned long long)r.p1, (unsigned long long)r.lf, r.g[0], r.g[1],
                    r.g[2], r.g[3], r.other);
        std::printf("  build_masks %016llx %016llx\n", (unsigned long long)m[0], (unsigned long long)m[1]);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const long n_random = argc > 1 ? std::atol(argv[1]) : 200000;
    // exactly 64 bytes on the heap: a read past the block is an ASan error
    std::vector<uint8_t> blk(64);
    uint8_t* b = blk.data();
    // every byte value at every position, alone (zeros around it) and among 'a'
    for (int bg = 0; bg < 2; ++bg)
        for (int pos = 0; pos < 64; ++pos)
            for (int v = 0; v < 256; ++v) {
                std::memset(b, bg ? 'a' : 0, 64);
                b[pos] = (uint8_t)v;
                check(b, bg ? "one byte among 'a'" : "one byte alone");
            }
    // 64 x '\n'
    std::memset(b, '\n', 64);
    check(b, "64 x LF");
    // random blocks of the bytes the staging pass tells apart
    static const uint8_t alphabet[8] = {'"', ' ', '\n', '\r', '\t', 0x7F, 0x80, 'a'};
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (long t = 0; t < n_random; ++t) {
        // (the first half sparse: mostly 'a', as a log line; the second half uniform)
        for (int i = 0; i < 64; ++i) {
            s ^= s << 13;
            s ^= s >> 7;
            s ^= s << 17;
            const unsigned r = (unsigned)(s >> 40);
            b[i] = t < n_random / 2 && (r >> 3) % 8 ? 'a' : alphabet[r & 7];
        }
        check(b, "random");
    }
    std::printf("stage_block_emu: %ld blocks checked, %d differ\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
