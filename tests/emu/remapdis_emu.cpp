// TEST-ONLY stand-alone program (its own main; built with ASan + UBSan by
// tests/test_remap_dissectors.py): the pure functions of the remapped-value
// dissectors -- screen_split, unique_id_decode, unique_id_ip of
// logparser_amd/csrc/lp_value.h, the header the table kernels and
// k_derived_lines include -- against a plain restatement with std::string,
// over every value of the input file (one per line)
//   * at every alignment 0..3 of a buffer with poisoned bytes around it, and
//   * at the very end of an exactly-sized heap buffer (a read past the value
//     is a heap-buffer-overflow under ASan).
// Prints "ok <checks>" and returns 0, or the first difference and 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../logparser_amd/csrc/lp_value.h"

namespace {

// String.split("x") with the trailing empty strings removed; false: no 'x'
bool ref_split(const std::string& v, std::vector<std::string>& parts) {
    parts.clear();
    if (v.find('x') == std::string::npos) return false;
    size_t s = 0;
    for (;;) {
        const size_t x = v.find('x', s);
        parts.push_back(v.substr(s, x == std::string::npos ? std::string::npos : x - s));
        if (x == std::string::npos) break;
        s = x + 1;
    }
    while (!parts.empty() && parts.back().empty()) parts.pop_back();
    return true;
}

// 24 letters of the URL-safe alphabet -> 18 bytes; false otherwise
bool ref_decode(const std::string& v, uint8_t b[18]) {
    static const char* const A = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_";
    if (v.size() != 24) return false;
    uint8_t bits[144];
    for (int k = 0; k < 24; ++k) {
        const char* p = v[k] ? strchr(A, v[k]) : nullptr;
        if (!p) return false;
        for (int q = 0; q < 6; ++q) bits[6 * k + q] = (uint8_t)(((p - A) >> (5 - q)) & 1);
    }
    for (int k = 0; k < 18; ++k) {
        b[k] = 0;
        for (int q = 0; q < 8; ++q) b[k] = (uint8_t)((b[k] << 1) | bits[8 * k + q]);
    }
    return true;
}

long long g_checks = 0;

bool check(const std::string& v, const uint8_t* p, const char* where) {
    const uint32_t n = (uint32_t)v.size();
    auto fail = [&](const char* what) {
        printf("MISMATCH %s (%s) on \"%s\"\n", what, where, v.c_str());
        return false;
    };
    std::vector<std::string> parts;
    const bool has = ref_split(v, parts);
    uint32_t wl = 0, ho = 0, hl = 0;
    const int got = lp::screen_split(p, n, wl, ho, hl);
    if (got != (has ? (int)parts.size() : -1)) return fail("screen_split count");
    if (got >= 1 && std::string((const char*)p, wl) != parts[0]) return fail("width");
    if (got >= 2 && (ho + hl > n || std::string((const char*)p + ho, hl) != parts[1])) return fail("height");
    uint8_t b[18];
    const bool dec = ref_decode(v, b);
    uint32_t f[5] = {0, 0, 0, 0, 0};
    if (lp::unique_id_decode(p, n, f) != dec) return fail("unique_id_decode validity");
    if (dec) {
        auto u32 = [&](int k) { return ((uint32_t)b[k] << 24) | ((uint32_t)b[k + 1] << 16) | ((uint32_t)b[k + 2] << 8) | b[k + 3]; };
        if (f[0] != u32(0) || f[1] != u32(4) || f[2] != u32(8) || f[3] != (((uint32_t)b[12] << 8) | b[13]) || f[4] != u32(14))
            return fail("unique_id_decode fields");
        char ip[15], want[32];
        const uint32_t m = lp::unique_id_ip(f[1], ip);
        const int wn = snprintf(want, sizeof want, "%u.%u.%u.%u", b[4], b[5], b[6], b[7]);
        if ((int)m != wn || memcmp(ip, want, m) != 0) return fail("unique_id_ip");
    }
    ++g_checks;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: remapdis_emu <values file>\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<std::string> values;
    for (std::string line; std::getline(in, line);) values.push_back(line);
    // the ip formatter's widths: every byte value in every position
    for (uint32_t x = 0; x < 256; ++x) {
        char ip[15], want[32];
        const uint32_t addr = (x << 24) | ((255 - x) << 16) | ((x * 7 & 255) << 8) | (x ^ 0x55);
        const uint32_t m = lp::unique_id_ip(addr, ip);
        const int wn = snprintf(want, sizeof want, "%u.%u.%u.%u", addr >> 24, (addr >> 16) & 255, (addr >> 8) & 255, addr & 255);
        if ((int)m != wn || memcmp(ip, want, m) != 0) { printf("MISMATCH unique_id_ip %08x\n", addr); return 1; }
    }
    for (const std::string& v : values) {
        for (int off = 0; off < 4; ++off) {
            std::vector<uint8_t> buf((size_t)off + v.size() + 8, (uint8_t)'x');  // 'x' around it: a read outside changes the split
            memcpy(buf.data() + off, v.data(), v.size());
            if (!check(v, buf.data() + off, "aligned buffer")) return 1;
            for (auto& c : buf) c = 'A';  // ... and letters: a read outside changes the decode
            memcpy(buf.data() + off, v.data(), v.size());
            if (!check(v, buf.data() + off, "aligned buffer")) return 1;
        }
        uint8_t* heap = new uint8_t[v.size() ? v.size() : 1];  // the value ends where the allocation ends
        const size_t pad = v.size() ? 0 : 1;
        memcpy(heap + pad, v.data(), v.size());
        const bool ok = check(v, heap + pad, "end of heap buffer");
        delete[] heap;
        if (!ok) return 1;
    }
    printf("ok %lld\n", g_checks);
    return 0;
}
