// TEST-ONLY stand-alone program (its own main; built with ASan + UBSan by
// tests/test_geoip_sanitizers.py): the MaxMind DB reader of
// logparser_amd/csrc/lp_mmdb.h and the address parser / tree walk of
// lp_geoip.h, the header k_geoip_lines includes.
//   mmdb_emu <values file> <database>...
//   * ip_parse on every value of the file (one per line) at the very end of an
//     exactly-sized heap buffer (a read past the value is a heap-buffer-overflow)
//     and through the kernel's staging (aligned 16-byte blocks, ip_align_words,
//     ip_parse_words) at every alignment 0..15; both against inet_pton, the
//     plain restatement of the decided subset: a value is decided exactly when
//     inet_pton accepts it, with the same bytes;
//   * the reader on every database: parse, every record's map walked to its
//     leaves, every value looked up;
//   * the same on systematically damaged copies of each database (truncated at
//     many lengths, bytes flipped and overwritten at a stride through the tree,
//     the data section and the metadata), each an exactly-sized heap buffer: a
//     copy is invalid or is walked like a good one, never a bad read.
// Prints "ok <values> <databases> <copies> <copies still valid>" and returns 0,
// or the first difference and 1.
#include <arpa/inet.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../logparser_amd/csrc/lp_mmdb.h"

using namespace lp;

namespace {

bool check_value(const std::string& v) {
    const uint32_t n = (uint32_t)v.size();
    uint8_t* heap = new uint8_t[n ? n : 1];
    memcpy(heap, v.data(), n);
    uint32_t a[4];
    const int fam = ip_parse(heap, n, a);
    delete[] heap;
    // inet_pton: the decided subset's plain restatement
    uint8_t b4[4], b6[16];
    int want = IPF_UNDECIDED;
    uint32_t w[4] = {0, 0, 0, 0};
    if (n <= (uint32_t)GEO_MAX_TEXT && inet_pton(AF_INET, v.c_str(), b4) == 1 && strlen(v.c_str()) == n) {
        want = IPF_V4;
        w[0] = ((uint32_t)b4[0] << 24) | ((uint32_t)b4[1] << 16) | ((uint32_t)b4[2] << 8) | b4[3];
    } else if (n <= (uint32_t)GEO_MAX_TEXT && inet_pton(AF_INET6, v.c_str(), b6) == 1 && strlen(v.c_str()) == n) {
        want = IPF_V6;
        for (int k = 0; k < 4; ++k)
            w[k] = ((uint32_t)b6[4 * k] << 24) | ((uint32_t)b6[4 * k + 1] << 16) | ((uint32_t)b6[4 * k + 2] << 8) | b6[4 * k + 3];
        if (w[0] == 0 && w[1] == 0 && w[2] == 0xFFFFu) {  // IPv4-mapped: an Inet4Address
            want = IPF_V4;
            w[0] = w[3];
            w[1] = w[2] = w[3] = 0;
        }
    }
    if (fam != want || memcmp(a, w, sizeof a) != 0) {
        printf("MISMATCH ip_parse \"%s\": family %d, inet_pton says %d\n", v.c_str(), fam, want);
        return false;
    }
    // the kernel's staging at every alignment: the text inside a 16-byte aligned 64-byte window
    if (n <= (uint32_t)GEO_MAX_TEXT)
        for (uint32_t m = 0; m < 16; ++m) {
            alignas(16) uint8_t win[64];
            memset(win, '7', sizeof win);  // digits around it: a read outside the text changes the answer
            memcpy(win + m, v.data(), n);
            uint32_t x[16], ww[12], a2[4];
            for (int j = 0; j < 4; ++j) {
                if (16u * (uint32_t)j < m + n) memcpy(x + 4 * j, win + 16 * j, 16);
                else memset(x + 4 * j, 0, 16);
            }
            ip_align_words(x, m, ww);
            if (ip_parse_words(ww, n, a2) != fam || memcmp(a, a2, sizeof a) != 0) {
                printf("MISMATCH staged ip_parse \"%s\" at alignment %u\n", v.c_str(), m);
                return false;
            }
        }
    return true;
}

// every value below the one at pos, pointers followed: false for a malformed one
bool walk_value(const mmdb::Section& S, size_t& pos, int depth) {
    if (depth > mmdb::MMDB_MAX_DEPTH) return false;
    mmdb::Val v;
    if (!mmdb::decode(S, pos, v)) return false;
    if (v.type == mmdb::T_MAP || v.type == mmdb::T_ARRAY) {
        size_t at = v.pos;
        const uint64_t items = (uint64_t)v.n * (v.type == mmdb::T_MAP ? 2 : 1);
        for (uint64_t k = 0; k < items; ++k)
            if (!walk_value(S, at, depth + 1)) return false;
        // (a container reached through a pointer ends elsewhere: pos stays after the pointer)
        if (at > pos && v.pos <= pos) pos = at;
    } else if (v.type == mmdb::T_UTF8 || v.type == mmdb::T_BYTES) {
        volatile uint8_t sink = 0;
        for (uint32_t k = 0; k < v.n; ++k) sink = sink ^ v.s[k];
    }
    return true;
}

// a parsed database: every record's map, a few keyed reads, every value looked up; the lookups' sum
uint64_t use_db(const mmdb::Db& D, const std::vector<std::string>& values) {
    uint64_t sum = 0;
    for (uint32_t off : D.rec_off) {
        size_t pos = off;
        walk_value(D.data, pos, 0);
        pos = off;
        mmdb::Val rec, city, names, en;
        bool found = false;
        if (mmdb::decode(D.data, pos, rec) && rec.type == mmdb::T_MAP && mmdb::map_get(D.data, rec, "city", city, found) &&
            found && mmdb::map_get(D.data, city, "names", names, found) && found &&
            mmdb::map_get(D.data, names, "en", en, found) && found && en.type == mmdb::T_UTF8)
            sum += en.n;
        mmdb::Val subs, last;
        if (rec.type == mmdb::T_MAP && mmdb::map_get(D.data, rec, "subdivisions", subs, found) && found &&
            subs.type == mmdb::T_ARRAY && subs.n && mmdb::array_get(D.data, subs, subs.n - 1, last))
            sum += last.n;
    }
    for (const std::string& v : values) {
        if (v.empty()) continue;
        const int64_t r = geo_lookup((const uint8_t*)v.data(), (uint32_t)v.size(), D.tree.data());
        if (r > (int64_t)D.rec_off.size()) { printf("record id out of range for \"%s\"\n", v.c_str()); return ~0ull; }
        sum += (uint64_t)(r + 1);
    }
    return sum;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: mmdb_emu <values file> <database>...\n"); return 2; }
    std::ifstream in(argv[1], std::ios::binary);
    if (!in) { printf("cannot read %s\n", argv[1]); return 2; }
    std::vector<std::string> values;
    for (std::string line; std::getline(in, line);) values.push_back(line);
    for (const std::string& v : values)
        if (!check_value(v)) return 1;
    // Double.toString of a few doubles the fixtures hold
    if (mmdb::java_double(52.5) != "52.5" || mmdb::java_double(5.75) != "5.75" || mmdb::java_double(1.0e-5) != "1.0E-5" ||
        mmdb::java_double(1.2345678e7) != "1.2345678E7" || mmdb::java_double(-0.0) != "-0.0" ||
        mmdb::java_double(100.0) != "100.0" || mmdb::java_double(0.001) != "0.001" || mmdb::java_double(-12.25) != "-12.25") {
        printf("MISMATCH java_double\n");
        return 1;
    }
    long long copies = 0, valid = 0;
    for (int k = 2; k < argc; ++k) {
        mmdb::Db D;
        std::string why;
        if (!mmdb::load(D, argv[k], why)) { printf("%s: %s\n", argv[k], why.c_str()); return 1; }
        if (use_db(D, values) == ~0ull) return 1;
        const std::vector<uint8_t> good = D.file;
        const size_t n = good.size();
        auto damaged = [&](std::vector<uint8_t> bytes) {
            mmdb::Db C;
            C.file.swap(bytes);
            C.file.shrink_to_fit();
            std::string w;
            ++copies;
            if (!mmdb::parse(C, w)) return true;
            ++valid;
            return use_db(C, values) != ~0ull;
        };
        // truncations: around both ends, and 24 lengths across the file
        for (size_t cut : {(size_t)0, (size_t)1, (size_t)13, (size_t)14, n - 1, n - 2, n - 20, n - 60, n - 120})
            if (cut < n && !damaged(std::vector<uint8_t>(good.begin(), good.begin() + (long)cut))) return 1;
        for (int q = 1; q <= 24 && n > 64; ++q)
            if (!damaged(std::vector<uint8_t>(good.begin(), good.begin() + (long)(n * (size_t)q / 25)))) return 1;
        // a byte damaged at a stride through the first 64 KiB, the last 4 KiB and in between: a bit
        // flipped, 0xFF (large sizes, pointers), 0x00
        const size_t stride = n > 400000 ? 997 : n / 90 + 1;
        for (size_t at = 0; at < n; at += (at > 65536 && at + 8192 < n) ? 65521 : stride)
            for (int mode = 0; mode < 3; ++mode) {
                std::vector<uint8_t> b = good;
                b[at] = mode == 0 ? (uint8_t)(b[at] ^ (1u << (at % 8))) : mode == 1 ? 0xFF : 0x00;
                if (n <= 400000 && at + 1 < n && mode == 1) b[at + 1] = 0xFF;
                if (!damaged(std::move(b))) return 1;
            }
    }
    printf("ok %zu %d %lld %lld\n", values.size(), argc - 2, copies, valid);
    return 0;
}
