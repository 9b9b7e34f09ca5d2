// TEST-ONLY stand-alone program (its own main): the core of the dictionary
// columns (logparser_amd/csrc/lp_dict.h: the hash, the probe / claim / min
// insert) on the CPU, built with ASan + UBSan (and ThreadSanitizer) and run
// directly by tests/test_table_dict.py.  An adversarial value set goes into
// one table single-threaded and from several std::threads, with the whole hash
// and with the hash narrowed to 1 and 2 bits; every run must leave, in each
// class's slot, the class's first row -- the same as a std::unordered_map
// built in row order.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../logparser_amd/csrc/lp_dict.h"

namespace {

std::vector<std::string> adversarial() {
    std::vector<std::string> v;
    const std::string pre(64, 'P');
    for (int rep = 0; rep < 3; ++rep) {
        v.push_back("");
        v.push_back("a");
        v.push_back("ab");
        v.push_back("abc");                  // prefixes of one another
        v.push_back("abcdefgh");             // exactly one word
        v.push_back("abcdefghi");
        v.push_back("abcdefgX");             // the last byte differs
        v.push_back(std::string(1, '\0'));   // a zero byte against the word's padding
        v.push_back(std::string(2, '\0'));
        v.push_back(std::string(8, '\0'));
        v.push_back(pre + "1");              // equal in the first 64 bytes
        v.push_back(pre + "2");
        v.push_back(pre);
        v.push_back(std::string(4096, 'B'));
        v.push_back(std::string(4095, 'B') + "C");
        for (int k = 0; k < 300; ++k) v.push_back("value-" + std::to_string(k * 7919 % 300));
        for (int k = 0; k < 40; ++k) v.push_back("GET");  // a hot key
    }
    return v;
}

uint64_t hash_of(const std::string& s) {
    return lp::dict_hash((uint32_t)s.size(), [&](uint32_t j) {
        uint64_t w = 0;
        const size_t o = 8 * (size_t)j;
        memcpy(&w, s.data() + o, s.size() - o < 8 ? s.size() - o : 8);
        return w;
    });
}

// rows [a, b) stepping by `step` into the table; returns false when a probe ran out
bool insert_rows(const std::vector<std::string>& v, std::vector<uint32_t>& slots, std::vector<uint32_t>& slot, int bits,
                 size_t a, size_t b, size_t step) {
    const uint32_t cap = (uint32_t)slots.size();
    bool ok = true;
    for (size_t k = a; k < b; k += step) {
        const std::string& x = v[k];
        const uint32_t s = lp::dict_insert<lp::DictAtHost>(slots.data(), cap, lp::dict_home(hash_of(x), cap, bits), (uint32_t)k,
                                                           [&](uint32_t r) { return v[r] == x; });
        slot[k] = s;
        ok = ok && s != lp::DICT_EMPTY;
    }
    return ok;
}

int run(const std::vector<std::string>& v, int bits, int threads) {
    const uint32_t cap = lp::dict_capacity((int64_t)v.size());
    std::vector<uint32_t> slots(cap, lp::DICT_EMPTY), slot(v.size(), lp::DICT_EMPTY);
    std::vector<char> ok((size_t)threads, 1);
    if (threads == 1) {
        ok[0] = insert_rows(v, slots, slot, bits, 0, v.size(), 1);
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t)  // interleaved rows: every class is contended
            pool.emplace_back([&, t] { ok[(size_t)t] = insert_rows(v, slots, slot, bits, (size_t)t, v.size(), (size_t)threads); });
        for (auto& th : pool) th.join();
    }
    int bad = 0;
    for (char c : ok) bad += c ? 0 : 1;
    std::unordered_map<std::string, uint32_t> first;
    for (size_t k = 0; k < v.size(); ++k) {
        const uint32_t want = first.emplace(v[k], (uint32_t)k).first->second;
        if (slot[k] >= cap || slots[slot[k]] != want) ++bad;
    }
    size_t used = 0;
    for (uint32_t s : slots) used += s != lp::DICT_EMPTY;
    if (used != first.size()) ++bad;  // one slot per class
    printf("bits %d threads %d: %zu rows, %zu classes, %d differ\n", bits, threads, v.size(), first.size(), bad);
    return bad;
}

}  // namespace

int main() {
    const std::vector<std::string> v = adversarial();
    int bad = 0;
    for (int bits : {0, 1, 2})
        for (int threads : {1, 4, 7})
            for (int rep = 0; rep < (threads == 1 ? 1 : 5); ++rep) bad += run(v, bits, threads);
    // a full table: the probe is bounded, the insert reports it
    {
        std::vector<uint32_t> slots(3, lp::DICT_EMPTY);
        const std::vector<std::string> w = {"a", "b", "c", "d"};
        uint32_t last = 0;
        for (uint32_t k = 0; k < 4; ++k)
            last = lp::dict_insert<lp::DictAtHost>(slots.data(), 3u, lp::dict_home(hash_of(w[k]), 3u, 0), k,
                                                   [&](uint32_t r) { return w[r] == w[k]; });
        if (last != lp::DICT_EMPTY) ++bad;
        printf("full table: %s\n", last == lp::DICT_EMPTY ? "reported" : "NOT reported");
    }
    printf("total: %d differ\n", bad);
    return bad ? 1 : 0;
}
