// TEST-ONLY stand-alone program (its own main): the pure value conversions of
// the typed table (logparser_amd/csrc/lp_value.h: digits, write_long,
// parse_long, decimal_to_double) on the CPU, built with ASan + UBSan and run
// directly by tests/test_value_edges.py.  Every function is compared with the
// C library on the values of a file (argv[1]: one "D <I.F>" / "L <text>" /
// "W <long>" line per value, the value-edge corpus) and on a few million
// seeded random ones: decimal_to_double against strtod by bit pattern,
// parse_long against strtoll behind Long.parseLong's syntax check, digits /
// write_long against snprintf.  Each input sits in a heap buffer of exactly
// its length, so a read past its end is an ASan report.
#include <cerrno>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../logparser_amd/csrc/lp_value.h"

namespace {

struct Count {
    long n = 0, bad = 0;
};

// the bytes of s in a heap block of exactly s.size() bytes (no terminator)
struct Exact {
    uint8_t* p;
    uint32_t n;
    explicit Exact(const std::string& s) : p((uint8_t*)malloc(s.size() ? s.size() : 1)), n((uint32_t)s.size()) {
        memcpy(p, s.data(), s.size());
    }
    ~Exact() { free(p); }
};

void check_decimal(const std::string& s, Count& c) {
    const Exact x(s);
    const double got = lp::decimal_to_double(x.p, x.n), want = strtod(s.c_str(), nullptr);
    uint64_t a, b;
    memcpy(&a, &got, 8);
    memcpy(&b, &want, 8);
    ++c.n;
    if (a != b) {
        if (c.bad++ < 10) printf("decimal_to_double(%s): %016" PRIx64 " want %016" PRIx64 "\n", s.c_str(), a, b);
    }
}

// Long.parseLong: [+-]?[0-9]+ within int64
bool ref_parse_long(const std::string& s, int64_t& out) {
    size_t k = !s.empty() && (s[0] == '+' || s[0] == '-') ? 1 : 0;
    if (k == s.size()) return false;
    for (size_t q = k; q < s.size(); ++q)
        if (s[q] < '0' || s[q] > '9') return false;
    errno = 0;
    const long long v = strtoll(s.c_str(), nullptr, 10);
    if (errno == ERANGE) return false;
    out = v;
    return true;
}

void check_parse(const std::string& s, Count& c) {
    const Exact x(s);
    int64_t got = 0, want = 0;
    const bool g = lp::parse_long(x.p, x.n, false, got), w = ref_parse_long(s, want);
    ++c.n;
    if (g != w || (g && got != want)) {
        if (c.bad++ < 10) printf("parse_long(%s): %d %" PRId64 " want %d %" PRId64 "\n", s.c_str(), (int)g, got, (int)w, want);
    }
    int64_t none = 7;
    if (lp::parse_long(x.p, x.n, true, none) || none != 7) ++c.bad;  // a leading '&': never a number
}

void check_write(int64_t l, Count& c) {
    char want[32];
    const int wn = snprintf(want, sizeof want, "%" PRId64, l);
    const uint32_t n = lp::digits(l);
    ++c.n;
    if ((int)n != wn) {
        if (c.bad++ < 10) printf("digits(%" PRId64 "): %u want %d\n", l, n, wn);
        return;
    }
    uint8_t* d = (uint8_t*)malloc(n);  // exactly the digits: a byte before or after is an ASan report
    lp::write_long(d, l, n);
    if (memcmp(d, want, n) != 0) {
        if (c.bad++ < 10) printf("write_long(%" PRId64 "): %.*s\n", l, (int)n, (const char*)d);
    }
    free(d);
}

std::string rand_digits(std::mt19937_64& g, int n) {
    std::string s((size_t)n, '0');
    for (char& ch : s) ch = (char)('0' + g() % 10);
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    Count dec, par, wr;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "r");
        if (!f) { printf("cannot read %s\n", argv[1]); return 2; }
        char line[512];
        while (fgets(line, sizeof line, f)) {
            std::string s(line);
            while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
            if (s.size() < 2 || s[1] != ' ') { printf("bad line: %s\n", s.c_str()); return 2; }
            const std::string v = s.substr(2);
            if (s[0] == 'D') check_decimal(v, dec);
            else if (s[0] == 'L') check_parse(v, par);
            else if (s[0] == 'W') check_write((int64_t)strtoll(v.c_str(), nullptr, 10), wr);
            else { printf("bad line: %s\n", s.c_str()); return 2; }
        }
        fclose(f);
        printf("file: %ld decimals, %ld texts, %ld longs\n", dec.n, par.n, wr.n);
    }
    std::mt19937_64 g(20261020);
    // I.F with 1-18 digits each side; every 8th a tie or near-tie at 2^53 .. 2^59
    static const char* const frac[] = {"0", "5", "50000000000000000", "500000000000000001", "499999999999999999", "25", "75"};
    for (int k = 0; k < 2000000; ++k) {
        if (k % 8 == 0) {
            const int e = 53 + (int)(g() % 7);
            const uint64_t i = (1ull << e) + (g() % 64) - 32;
            check_decimal(std::to_string(i) + "." + frac[g() % 7], dec);
        } else {
            check_decimal(rand_digits(g, 1 + (int)(g() % 18)) + "." + rand_digits(g, 1 + (int)(g() % 18)), dec);
        }
    }
    // longs of every bit length, both signs, and the ends
    for (int k = 0; k < 1000000; ++k) {
        const uint64_t u = g() >> (g() % 64);
        check_write((int64_t)u, wr);
        check_write((int64_t)(0 - u), wr);
    }
    for (int64_t l : {(int64_t)0, (int64_t)9, (int64_t)10, (int64_t)-1, (int64_t)-9, (int64_t)-10, INT64_MAX, INT64_MIN,
                      INT64_MIN + 1, (int64_t)1 << 61, ((int64_t)1 << 61) - 1, -((int64_t)1 << 61), -((int64_t)1 << 61) - 1})
        check_write(l, wr);
    // texts: digit strings of 1-22 digits with and without a sign, around 2^63, and broken ones
    for (int k = 0; k < 1000000; ++k) {
        std::string s;
        const uint64_t r = g();
        if (r % 4 == 0) s = "+";
        else if (r % 4 == 1) s = "-";
        if ((r >> 2) % 8 == 0) s += std::to_string(0x7FFFFFFFFFFFFFF0ull + (r >> 8) % 32);  // 2^63 - 16 .. 2^63 + 15
        else s += rand_digits(g, 1 + (int)((r >> 8) % 22));
        if ((r >> 16) % 64 == 0) s[(r >> 24) % s.size()] = "x -+.:"[(r >> 32) % 6];
        check_parse(s, par);
    }
    for (const char* s : {"", "+", "-", "+-1", "--1", "1-", "0", "-0", "+0", "00000000000000000000000000000000000012",
                          "9223372036854775807", "9223372036854775808", "-9223372036854775808", "-9223372036854775809",
                          "18446744073709551616", "99999999999999999999"})
        check_parse(s, par);
    printf("decimal_to_double: %ld values, %ld differ\n", dec.n, dec.bad);
    printf("parse_long: %ld values, %ld differ\n", par.n, par.bad);
    printf("digits / write_long: %ld values, %ld differ\n", wr.n, wr.bad);
    const long bad = dec.bad + par.bad + wr.bad;
    printf("total: %ld differ\n", bad);
    return bad ? 1 : 0;
}
