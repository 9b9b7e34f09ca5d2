// The host core of the Arrow C Data Interface export (include/logparser_amd.h
// lp_arrow_from_tables): the validity bit-packing, and the ArrowSchema /
// ArrowArray trees with their release callbacks and the shared ownership of
// the buffers behind them.  Plain C++ without HIP: arrow_export.cpp builds the
// library's entry points on it, tests/emu/arrow_emu.cpp runs it stand-alone
// under the sanitizers.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/logparser_amd.h"

namespace lp {
namespace arrow {

// Bytes of a validity bitmap of n rows: Arrow's bit per row, allocated in
// multiples of 64 bytes (every bit past n is 0)
inline size_t bitmap_bytes(int64_t n) { return ((((size_t)n + 7) >> 3) + 63) & ~(size_t)63; }

// valid[0, n) (a byte per row, any non-zero value is "valid") -> bitmap: bit
// k & 7 of byte k >> 3.  Writes all bitmap_bytes(n) bytes; returns the number
// of valid rows (null_count = n - that).
inline int64_t pack_validity(const uint8_t* valid, int64_t n, uint8_t* bitmap) {
    const size_t bytes = bitmap_bytes(n);
    int64_t set = 0, k = 0;
    size_t b = 0;
    for (; k + 8 <= n; k += 8, ++b) {
        uint64_t w;
        memcpy(&w, valid + k, 8);
        // the high bit of every non-zero byte, then the eight of them into one byte
        const uint64_t hb = (((w & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | w) & 0x8080808080808080ull;
        const uint8_t m = (uint8_t)(((hb >> 7) * 0x0102040810204080ull) >> 56);
        bitmap[b] = m;
        set += __builtin_popcount(m);
    }
    if (k < n) {
        uint8_t m = 0;
        for (int q = 0; k + q < n; ++q) m |= (uint8_t)((valid[k + q] != 0 ? 1u : 0u) << q);
        bitmap[b++] = m;
        set += __builtin_popcount(m);
    }
    if (b < bytes) memset(bitmap + b, 0, bytes - b);
    return set;
}

// What every exported ARRAY structure of one batch shares: the buffers this
// library allocated for it (bitmaps, narrowed offsets; a host deep copy: all
// of them) and the caller's owner.  The last structure released frees them and
// calls the owner, once.
struct Shared {
    std::atomic<int64_t> refs{0};
    lp_arrow_owner owner{nullptr, nullptr};
    std::vector<void*> owned;
    void (*free_buf)(void*) = nullptr;
};
inline void shared_unref(Shared* sh) {
    if (sh->refs.fetch_sub(1) != 1) return;
    for (void* p : sh->owned)
        if (p) sh->free_buf(p);
    if (sh->owner.free_fn) sh->owner.free_fn(sh->owner.ctx);
    delete sh;
}

// private_data of one ArrowArray.  The children's and the dictionary's
// STRUCTURES are this node's memory; what they point to is released through
// their own callbacks -- unless the consumer moved them out (release NULL),
// then the moved copy releases it whenever the consumer likes.
struct ANode {
    Shared* sh = nullptr;
    const void* bufs[3] = {nullptr, nullptr, nullptr};
    std::vector<ArrowArray*> kids;
    ArrowArray* dict = nullptr;
};
inline void release_array(ArrowArray* a) {
    if (!a || !a->release) return;
    ANode* n = static_cast<ANode*>(a->private_data);
    for (ArrowArray* k : n->kids) {
        if (k->release) k->release(k);
        delete k;
    }
    if (n->dict) {
        if (n->dict->release) n->dict->release(n->dict);
        delete n->dict;
    }
    Shared* sh = n->sh;
    delete n;
    a->release = nullptr;
    shared_unref(sh);
}
inline void make_array(ArrowArray* a, Shared* sh, int64_t length, int64_t nulls, int n_buffers, const void* b0,
                       const void* b1, const void* b2, std::vector<ArrowArray*> kids = {}, ArrowArray* dict = nullptr) {
    ANode* n = new ANode;
    n->sh = sh;
    n->bufs[0] = b0;
    n->bufs[1] = b1;
    n->bufs[2] = b2;
    n->kids = std::move(kids);
    n->dict = dict;
    sh->refs.fetch_add(1);
    a->length = length;
    a->null_count = nulls;
    a->offset = 0;
    a->n_buffers = n_buffers;
    a->n_children = (int64_t)n->kids.size();
    a->buffers = n->bufs;
    a->children = n->kids.empty() ? nullptr : n->kids.data();
    a->dictionary = dict;
    a->release = release_array;
    a->private_data = n;
}

struct SNode {
    std::string format, name;
    std::vector<ArrowSchema*> kids;
    ArrowSchema* dict = nullptr;
};
inline void release_schema(ArrowSchema* s) {
    if (!s || !s->release) return;
    SNode* n = static_cast<SNode*>(s->private_data);
    for (ArrowSchema* k : n->kids) {
        if (k->release) k->release(k);
        delete k;
    }
    if (n->dict) {
        if (n->dict->release) n->dict->release(n->dict);
        delete n->dict;
    }
    delete n;
    s->release = nullptr;
}
inline void make_schema(ArrowSchema* s, const char* format, const char* name, int64_t flags,
                        std::vector<ArrowSchema*> kids = {}, ArrowSchema* dict = nullptr) {
    SNode* n = new SNode;
    n->format = format;
    n->name = name ? name : "";
    n->kids = std::move(kids);
    n->dict = dict;
    s->format = n->format.c_str();
    s->name = n->name.c_str();
    s->metadata = nullptr;
    s->flags = flags;
    s->n_children = (int64_t)n->kids.size();
    s->children = n->kids.empty() ? nullptr : n->kids.data();
    s->dictionary = dict;
    s->release = release_schema;
    s->private_data = n;
}

// One column of a batch: the table call's column and what the packaging made
// for it (bitmap: null when the column has no nulls; off32: a map's narrowed
// entry offsets).
struct Col {
    int form = LP_ARROW_PLAIN;
    const lp_table_col* plain = nullptr;
    const lp_table_dict_col* dict = nullptr;
    const lp_table_map_col* map = nullptr;
    const char* name = nullptr;
    const uint8_t* bitmap = nullptr;
    int64_t nulls = 0;
    const int32_t* off32 = nullptr;
};

// The Arrow format of a plain column: "@line" is large_binary, its bytes are not validated
inline const char* plain_format(const lp_table_col& c) {
    if (c.kind == LP_CAST_LONG) return "l";
    if (c.kind == LP_CAST_DOUBLE) return "g";
    return c.path && strcmp(c.path, "@line") == 0 ? "Z" : "U";
}

// (a string array's data pointer is never null on the host, even without bytes)
inline const void* data_or(const void* p, bool host) {
    static const char empty[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    return p || !host ? p : (const void*)empty;
}

// The record batch of cols (each n_rows long): the struct array and its schema
inline void build_batch(int64_t n_rows, const std::vector<Col>& cols, bool host, Shared* sh, ArrowSchema* schema,
                        ArrowArray* array) {
    std::vector<ArrowSchema*> skids;
    std::vector<ArrowArray*> akids;
    for (const Col& c : cols) {
        ArrowSchema* s = new ArrowSchema;
        ArrowArray* a = new ArrowArray;
        if (c.form == LP_ARROW_PLAIN) {
            const lp_table_col& p = *c.plain;
            make_schema(s, plain_format(p), c.name, ARROW_FLAG_NULLABLE);
            if (p.kind == LP_CAST_STRING) make_array(a, sh, n_rows, c.nulls, 3, c.bitmap, p.i64, data_or(p.chars, host));
            else make_array(a, sh, n_rows, c.nulls, 2, c.bitmap, p.kind == LP_CAST_LONG ? (const void*)p.i64 : (const void*)p.f64, nullptr);
        } else if (c.form == LP_ARROW_DICT) {
            const lp_table_dict_col& d = *c.dict;
            ArrowSchema* ds = new ArrowSchema;
            ArrowArray* da = new ArrowArray;
            make_schema(ds, "U", "", 0);
            make_array(da, sh, d.dict_len, 0, 3, nullptr, d.dict_off, data_or(d.dict_chars, host));
            make_schema(s, "i", c.name, ARROW_FLAG_NULLABLE, {}, ds);
            make_array(a, sh, n_rows, c.nulls, 2, c.bitmap, data_or(d.index, host), nullptr, {}, da);
        } else {
            const lp_table_map_col& m = *c.map;
            const int64_t ne = (int64_t)m.entries_len;
            ArrowSchema *ks = new ArrowSchema, *vs = new ArrowSchema, *es = new ArrowSchema;
            ArrowArray *ka = new ArrowArray, *va = new ArrowArray, *ea = new ArrowArray;
            make_schema(ks, "U", "key", 0);
            make_schema(vs, "U", "value", ARROW_FLAG_NULLABLE);
            make_schema(es, "+s", "entries", 0, {ks, vs});
            make_array(ka, sh, ne, 0, 3, nullptr, m.key_off, data_or(m.key_chars, host));
            make_array(va, sh, ne, 0, 3, nullptr, m.val_off, data_or(m.val_chars, host));
            make_array(ea, sh, ne, 0, 1, nullptr, nullptr, nullptr, {ka, va});
            make_schema(s, "+m", c.name, ARROW_FLAG_NULLABLE, {es});
            make_array(a, sh, n_rows, c.nulls, 2, c.bitmap, c.off32, nullptr, {ea});
        }
        skids.push_back(s);
        akids.push_back(a);
    }
    make_schema(schema, "+s", "", 0, std::move(skids));
    make_array(array, sh, n_rows, 0, 1, nullptr, nullptr, nullptr, std::move(akids));
}

}  // namespace arrow

// lp_arrow_from_tables with the children in a chosen order (lp_result_arrow's:
// the order of its columns): order[k] indexes the plain columns, then the
// dictionary columns, then the maps (null: that order).  pack_ms (may be null):
// HIP-event ms of the packaging kernels of a device export.
int arrow_wrap(int device, void* stream, int64_t n_rows, const lp_table_col* plain, const char* const* plain_names,
               int n_plain, const lp_table_dict_col* dict, const char* const* dict_names, int n_dict,
               const lp_table_map_col* map, const char* const* map_names, int n_map, const int* order,
               const lp_arrow_owner* owner, ArrowSchema* schema_out, ArrowDeviceArray* array_out, float* pack_ms);

}  // namespace lp
