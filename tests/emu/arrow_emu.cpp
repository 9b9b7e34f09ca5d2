// Stand-alone program over the host core of the Arrow export
// (logparser_amd/csrc/lp_arrow.h), built with -fsanitize=address,undefined and
// run directly (tests/test_arrow_export.py):
//   - pack_validity against a per-bit loop for every n in [0, 1100], several
//     patterns, valid bytes of 1 / 2 / 255, the source at every byte skew 0..15;
//     source and bitmap are heap blocks of exactly their size, so a read or a
//     write past either end is an ASan report;
//   - record batches of every column form built with build_batch and released
//     in every order (schema first, array first, a child moved out, the
//     dictionary column moved out, every child moved out), every buffer walked
//     to its computed size, the owner counted: 0 before the last array
//     structure is released, 1 after; the leak check is on.
#include <cstdio>
#include <memory>
#include <random>

#include "../../logparser_amd/csrc/lp_arrow.h"

namespace A = lp::arrow;

static long g_differ = 0;
static int g_owner = 0;
static void owner_fn(void* ctx) { ++*static_cast<int*>(ctx); }

static void check(bool ok, const char* what, long a = 0, long b = 0) {
    if (ok) return;
    ++g_differ;
    printf("DIFFER %s (%ld, %ld)\n", what, a, b);
}

static void bitpack_case(int64_t n, int pattern, int skew, std::mt19937& rng) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[(size_t)n + (size_t)skew + 1]);  // (+1: never a zero-size new)
    uint8_t* valid = block.get() + skew;
    static const uint8_t vals[4] = {1, 2, 255, 128};
    for (int64_t k = 0; k < n; ++k) {
        bool v = true;
        switch (pattern) {
            case 0: v = true; break;
            case 1: v = false; break;
            case 2: v = k != 0; break;
            case 3: v = k != n - 1; break;
            case 4: v = k % 3 != 0; break;
            default: v = (rng() & 3u) != 0; break;
        }
        valid[k] = v ? vals[rng() & 3u] : 0;
    }
    const size_t bytes = A::bitmap_bytes(n);
    check(bytes % 64 == 0 && bytes * 8 >= (size_t)n, "bitmap_bytes", n, (long)bytes);
    std::unique_ptr<uint8_t[]> bm(new uint8_t[bytes + 1]);
    memset(bm.get(), 0xA5, bytes);
    const int64_t set = A::pack_validity(valid, n, bm.get());
    int64_t want = 0;
    for (size_t bit = 0; bit < bytes * 8; ++bit) {
        const bool w = (int64_t)bit < n && valid[bit] != 0;
        want += w ? 1 : 0;
        if ((((bm[bit >> 3] >> (bit & 7)) & 1) != 0) != w) {
            check(false, "bit", n, (long)bit);
            break;
        }
    }
    check(set == want, "count", set, want);
}

// One batch of every form in heap blocks of exactly the computed sizes
struct Batch {
    int64_t n;
    std::vector<uint8_t> v_long, v_dbl, v_str, v_line, v_dict, v_map;
    std::vector<int64_t> longs, s_off, l_off, d_off, e_off, k_off, m_off;
    std::vector<double> dbls;
    std::vector<char> s_chars, l_chars, d_chars, k_chars, m_chars;
    std::vector<int32_t> index;
    lp_table_col plain[4];
    lp_table_dict_col dict;
    lp_table_map_col map;
    explicit Batch(int64_t rows, bool all_valid) : n(rows) {
        auto val = [&](int64_t k, int m) { return (uint8_t)(all_valid || k % m != 0 ? 1 + (k & 1) : 0); };
        for (int64_t k = 0; k < n; ++k) {
            v_long.push_back(val(k, 2));
            v_dbl.push_back(val(k, 3));
            v_str.push_back(val(k, 4));
            v_line.push_back(1);
            v_dict.push_back(val(k, 5));
            v_map.push_back(val(k, 6));
            longs.push_back(k * 7);
            dbls.push_back(k * 0.5);
            index.push_back(v_dict.back() ? (int32_t)(k % 3) : 0);
        }
        auto strings = [&](std::vector<int64_t>& off, std::vector<char>& chars, int64_t count, int len) {
            off.push_back(0);
            for (int64_t k = 0; k < count; ++k) {
                for (int q = 0; q < (int)((k * 5 + len) % 7); ++q) chars.push_back((char)('a' + (k + q) % 26));
                off.push_back((int64_t)chars.size());
            }
        };
        strings(s_off, s_chars, n, 1);
        strings(l_off, l_chars, n, 2);
        strings(d_off, d_chars, 3, 3);
        e_off.push_back(0);
        for (int64_t k = 0; k < n; ++k) e_off.push_back(e_off.back() + (v_map[(size_t)k] ? k % 4 : 0));
        strings(k_off, k_chars, e_off.back(), 4);
        strings(m_off, m_chars, e_off.back(), 5);
        memset(plain, 0, sizeof plain);
        plain[0] = lp_table_col{"BYTES:x", LP_CAST_LONG, v_long.data(), longs.data(), nullptr, nullptr, 0, 0};
        plain[1] = lp_table_col{"SECONDS:y", LP_CAST_DOUBLE, v_dbl.data(), nullptr, dbls.data(), nullptr, 0, 0};
        plain[2] = lp_table_col{"STRING:z", LP_CAST_STRING, v_str.data(), s_off.data(), nullptr, s_chars.data(), s_chars.size(), s_chars.size()};
        plain[3] = lp_table_col{"@line", LP_CAST_STRING, v_line.data(), l_off.data(), nullptr, l_chars.data(), l_chars.size(), l_chars.size()};
        dict = lp_table_dict_col{"STRING:d", v_dict.data(), index.data(), d_off.data(), d_chars.data(), 3, d_chars.size(), 3, d_chars.size()};
        map = lp_table_map_col{};
        map.path = "STRING:q.*";
        map.valid = v_map.data();
        map.entry_off = e_off.data();
        map.key_off = k_off.data();
        map.val_off = m_off.data();
        map.key_chars = k_chars.data();
        map.val_chars = m_chars.data();
        map.entries_len = map.entries_cap = (uint64_t)e_off.back();
        map.key_chars_len = k_chars.size();
        map.val_chars_len = m_chars.size();
    }
};

// The export of B: what lp_arrow_from_tables does on host memory
static void export_batch(const Batch& B, ArrowSchema* schema, ArrowArray* array) {
    std::vector<A::Col> cols;
    A::Shared* sh = new A::Shared;
    sh->free_buf = free;
    sh->owner = lp_arrow_owner{owner_fn, &g_owner};
    auto pack = [&](A::Col& C, const uint8_t* valid) {
        uint8_t* bm = (uint8_t*)malloc(A::bitmap_bytes(B.n) + 64);
        const int64_t set = B.n > 0 ? A::pack_validity(valid, B.n, bm) : 0;
        C.nulls = B.n - set;
        if (C.nulls == 0) {
            free(bm);
            bm = nullptr;
        } else {
            sh->owned.push_back(bm);
        }
        C.bitmap = bm;
    };
    for (int c = 0; c < 4; ++c) {
        A::Col C;
        C.form = LP_ARROW_PLAIN;
        C.plain = &B.plain[c];
        C.name = B.plain[c].path;
        pack(C, B.plain[c].valid);
        cols.push_back(C);
    }
    {
        A::Col C;
        C.form = LP_ARROW_DICT;
        C.dict = &B.dict;
        C.name = "d";
        pack(C, B.dict.valid);
        cols.push_back(C);
    }
    {
        A::Col C;
        C.form = LP_ARROW_MAP;
        C.map = &B.map;
        C.name = "q";
        pack(C, B.map.valid);
        int32_t* o = (int32_t*)malloc(4 * ((size_t)B.n + 1));
        for (int64_t k = 0; k <= B.n; ++k) o[k] = (int32_t)B.map.entry_off[k];
        sh->owned.push_back(o);
        C.off32 = o;
        cols.push_back(C);
    }
    A::build_batch(B.n, cols, true, sh, schema, array);
}

// Every buffer of a, read to the size its format gives it; returns a checksum
static uint64_t walk(const ArrowSchema* s, const ArrowArray* a) {
    uint64_t sum = 0;
    auto bytes = [&](const void* p, size_t n) {
        const uint8_t* q = static_cast<const uint8_t*>(p);
        for (size_t k = 0; k < n; ++k) sum += q[k];
    };
    const std::string f = s->format;
    const size_t n = (size_t)a->length;
    check(a->offset == 0 && a->release != nullptr && a->n_children == s->n_children, "array shape");
    if (a->buffers[0]) {
        bytes(a->buffers[0], A::bitmap_bytes(a->length));
        check(a->null_count > 0, "a bitmap without nulls");
    } else {
        check(a->null_count == 0, "nulls without a bitmap");
    }
    if (f == "l" || f == "g") bytes(a->buffers[1], 8 * n);
    else if (f == "i") bytes(a->buffers[1], 4 * n);
    else if (f == "U" || f == "Z") {
        bytes(a->buffers[1], 8 * (n + 1));
        bytes(a->buffers[2], (size_t)static_cast<const int64_t*>(a->buffers[1])[n]);
    } else if (f == "+m") bytes(a->buffers[1], 4 * (n + 1));
    else check(f == "+s", "format");
    for (int64_t k = 0; k < a->n_children; ++k) sum += walk(s->children[k], a->children[k]);
    if (a->dictionary) sum += walk(s->dictionary, a->dictionary);
    return sum;
}

// Move a structure out of its parent as a consumer does: copy it, mark the source released
static ArrowArray move_out(ArrowArray* src) {
    ArrowArray m = *src;
    src->release = nullptr;
    return m;
}

static void release_orders(int64_t n, bool all_valid) {
    const Batch B(n, all_valid);
    uint64_t sum0 = 0;
    for (int order = 0; order < 5; ++order) {
        ArrowSchema schema;
        ArrowArray array;
        g_owner = 0;
        export_batch(B, &schema, &array);
        check(std::string(schema.format) == "+s" && schema.n_children == 6 && array.n_children == 6 && array.length == n, "top");
        check(std::string(schema.children[3]->format) == "Z" && std::string(schema.children[2]->format) == "U", "formats");
        check(schema.children[4]->dictionary && !(schema.children[4]->flags & ARROW_FLAG_DICTIONARY_ORDERED), "dictionary");
        check(std::string(schema.children[5]->format) == "+m" && schema.children[5]->children[0]->flags == 0 &&
                  schema.children[5]->children[0]->children[1]->flags == ARROW_FLAG_NULLABLE, "map");
        if (all_valid)
            for (int c = 0; c < 6; ++c) check(array.children[c]->buffers[0] == nullptr && array.children[c]->null_count == 0, "all valid");
        const uint64_t sum = walk(&schema, &array);
        if (order == 0) sum0 = sum;
        check(sum == sum0, "walk checksum");
        if (order == 0) {  // schema first
            schema.release(&schema);
            check(schema.release == nullptr && g_owner == 0, "schema first", g_owner);
            array.release(&array);
        } else if (order == 1) {  // array first
            array.release(&array);
            check(array.release == nullptr && g_owner == 1, "array first", g_owner);
            schema.release(&schema);
        } else if (order == 2) {  // one child moved out, released after its parent
            ArrowArray kid = move_out(array.children[2]);
            array.release(&array);
            check(g_owner == 0, "moved child keeps the owner", g_owner);
            schema.release(&schema);
            check(g_owner == 0, "the schema holds no buffer", g_owner);
            kid.release(&kid);
        } else if (order == 3) {  // the dictionary column moved out: its dictionary goes through it
            ArrowArray kid = move_out(array.children[4]);
            ArrowSchema skid = *schema.children[4];
            schema.children[4]->release = nullptr;
            schema.release(&schema);
            array.release(&array);
            check(g_owner == 0, "moved dictionary column keeps the owner", g_owner);
            check(kid.dictionary && kid.dictionary->length == 3, "dictionary of the moved column");
            walk(&skid, &kid);
            kid.release(&kid);
            skid.release(&skid);
        } else {  // every child moved out, released before and after the parent
            std::vector<ArrowArray> kids;
            for (int c = 0; c < 6; ++c) kids.push_back(move_out(array.children[c]));
            for (int c = 0; c < 3; ++c) kids[(size_t)c].release(&kids[(size_t)c]);
            array.release(&array);
            check(g_owner == 0, "moved children keep the owner", g_owner);
            for (int c = 3; c < 6; ++c) {
                check(g_owner == 0, "before the last child", g_owner);
                kids[(size_t)c].release(&kids[(size_t)c]);
            }
            schema.release(&schema);
        }
        check(g_owner == 1, "owner called once", g_owner);
    }
}

int main() {
    static_assert(sizeof(ArrowSchema) == 72 && sizeof(ArrowArray) == 80 && sizeof(ArrowDeviceArray) == 128, "the ABI's sizes");
    printf("sizes: %zu %zu %zu\n", sizeof(ArrowSchema), sizeof(ArrowArray), sizeof(ArrowDeviceArray));
    std::mt19937 rng(20261020);
    long cases = 0;
    for (int64_t n = 0; n <= 1100; ++n)
        for (int pattern = 0; pattern < 7; ++pattern, ++cases) bitpack_case(n, pattern, (int)((n + pattern) & 15), rng);
    for (int64_t n : {0, 1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 4097, 8193})
        for (int skew = 0; skew < 16; ++skew, ++cases) bitpack_case(n, 5, skew, rng);
    printf("bit-packing: %ld cases\n", cases);
    for (int64_t n : {0, 1, 7, 64, 65, 513, 1100}) {
        release_orders(n, false);
        release_orders(n, true);
    }
    printf("release orders: 5 x 14 batches\n");
    printf("total: %ld differ\n", g_differ);
    return g_differ ? 1 : 0;
}
