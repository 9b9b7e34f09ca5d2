// Arrow C Data Interface export (include/logparser_amd.h): lp_arrow_from_tables
// -- the packaging of columns the table calls filled into an ArrowSchema and an
// ArrowDeviceArray -- and lp_arrow_to_host.  The structures, their release
// callbacks and the host bit-packing are lp_arrow.h (no HIP); here are the
// argument checks, the allocation of what the packaging adds (bitmaps, narrowed
// map offsets) and, for device memory, the launches of arrow.hip's kernels.
// lp_result_arrow (capi.cpp) fills the columns through the table calls' own
// paths and hands them to arrow_wrap.
#include <hip/hip_runtime.h>

#include <new>
#include <string>
#include <vector>

#include "kernels.h"
#include "lp_arrow.h"

namespace lp {
namespace {

void hip_free_buf(void* p) { (void)hipFree(p); }

// Is p memory of device (what the kernels may dereference)?
bool on_device(int device, const void* p) {
    hipPointerAttribute_t a{};
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (an unregistered host pointer: not a sticky error)
        return false;
    }
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) && a.device == device;
}

void clear_outputs(ArrowSchema* schema, ArrowDeviceArray* array) {
    if (schema) memset(schema, 0, sizeof *schema);
    if (array) memset(array, 0, sizeof *array);
}

// What the packaging allocated before the structures took it over
struct Scratch {
    bool host;
    std::vector<void*> bufs;
    void* get(size_t bytes) {
        void* p = nullptr;
        if (bytes == 0) bytes = 64;
        if (host) p = malloc(bytes);
        else if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
        if (p) bufs.push_back(p);
        return p;
    }
    void drop(void* p) {
        for (void*& q : bufs)
            if (q == p) {
                if (host) free(q);
                else (void)hipFree(q);
                q = nullptr;
            }
    }
    void drop_all() {
        for (void* q : bufs)
            if (q) drop(q);
        bufs.clear();
    }
};

}  // namespace

int arrow_wrap(int device, void* stream, int64_t n_rows, const lp_table_col* plain, const char* const* plain_names,
               int n_plain, const lp_table_dict_col* dict, const char* const* dict_names, int n_dict,
               const lp_table_map_col* map, const char* const* map_names, int n_map, const int* order,
               const lp_arrow_owner* owner, ArrowSchema* schema_out, ArrowDeviceArray* array_out, float* pack_ms) {
    clear_outputs(schema_out, array_out);
    if (!schema_out || !array_out || n_rows < 0 || n_plain < 0 || n_dict < 0 || n_map < 0) return LP_E_INVALID;
    const int n_cols = n_plain + n_dict + n_map;
    if (n_cols <= 0 || (n_plain && !plain) || (n_dict && !dict) || (n_map && !map)) return LP_E_INVALID;
    const bool host = device < 0;
    // the columns in plain / dictionary / map order, every argument checked before anything is read
    std::vector<arrow::Col> cols((size_t)n_cols);
    std::vector<const uint8_t*> valid((size_t)n_cols, nullptr);
    for (int c = 0; c < n_cols; ++c) {
        arrow::Col& C = cols[(size_t)c];
        const char* name = nullptr;
        if (c < n_plain) {
            const lp_table_col& p = plain[c];
            C.form = LP_ARROW_PLAIN;
            C.plain = &p;
            name = plain_names && plain_names[c] ? plain_names[c] : p.path;
            valid[(size_t)c] = p.valid;
            if (p.kind != LP_CAST_STRING && p.kind != LP_CAST_LONG && p.kind != LP_CAST_DOUBLE) return LP_E_INVALID;
            if (p.kind == LP_CAST_STRING ? !p.i64 : n_rows > 0 && (p.kind == LP_CAST_LONG ? !p.i64 : !p.f64)) return LP_E_INVALID;
            if (p.kind == LP_CAST_STRING && p.chars_len > 0 && !p.chars) return LP_E_INVALID;
        } else if (c < n_plain + n_dict) {
            const lp_table_dict_col& d = dict[c - n_plain];
            C.form = LP_ARROW_DICT;
            C.dict = &d;
            name = dict_names && dict_names[c - n_plain] ? dict_names[c - n_plain] : d.path;
            valid[(size_t)c] = d.valid;
            if (!d.dict_off || d.dict_len < 0 || d.dict_len > 0x7FFFFFFF || (n_rows > 0 && !d.index) ||
                (d.dict_chars_len > 0 && !d.dict_chars))
                return LP_E_INVALID;
        } else {
            const lp_table_map_col& m = map[c - n_plain - n_dict];
            C.form = LP_ARROW_MAP;
            C.map = &m;
            name = map_names && map_names[c - n_plain - n_dict] ? map_names[c - n_plain - n_dict] : m.path;
            valid[(size_t)c] = m.valid;
            if (m.entries_len > 0x7FFFFFFFull) return LP_E_INVALID;  // Arrow's map has int32 offsets: build it in windows
            if (!m.entry_off || !m.key_off || !m.val_off || (m.key_chars_len > 0 && !m.key_chars) ||
                (m.val_chars_len > 0 && !m.val_chars))
                return LP_E_INVALID;
        }
        if (!name || (n_rows > 0 && !valid[(size_t)c])) return LP_E_INVALID;
        C.name = name;
    }
    if (order) {  // a permutation of the columns
        std::vector<char> seen((size_t)n_cols, 0);
        for (int k = 0; k < n_cols; ++k) {
            if (order[k] < 0 || order[k] >= n_cols || seen[(size_t)order[k]]) return LP_E_INVALID;
            seen[(size_t)order[k]] = 1;
        }
    }
    Scratch S{host, {}};
    const size_t bm_bytes = arrow::bitmap_bytes(n_rows);
    std::vector<uint8_t*> bitmap((size_t)n_cols, nullptr);
    std::vector<int64_t> n_valid((size_t)n_cols, 0);
    auto fail = [&](int rc) {
        S.drop_all();
        return rc;
    };
    if (n_rows > 0)
        for (int c = 0; c < n_cols; ++c)
            if (!(bitmap[(size_t)c] = (uint8_t*)S.get(bm_bytes))) return fail(LP_E_NOMEM);
    for (int c = n_plain + n_dict; c < n_cols; ++c)
        if (!(cols[(size_t)c].off32 = (int32_t*)S.get(4 * ((size_t)n_rows + 1)))) return fail(LP_E_NOMEM);
    if (host) {
        for (int c = 0; c < n_cols; ++c) {
            if (n_rows > 0) n_valid[(size_t)c] = arrow::pack_validity(valid[(size_t)c], n_rows, bitmap[(size_t)c]);
            if (cols[(size_t)c].form == LP_ARROW_MAP) {
                int32_t* o = const_cast<int32_t*>(cols[(size_t)c].off32);
                const int64_t* e = cols[(size_t)c].map->entry_off;
                for (int64_t k = 0; k <= n_rows; ++k) o[k] = (int32_t)e[k];
            }
        }
    } else {
        if (hipSetDevice(device) != hipSuccess) return fail(LP_E_DEVICE);
        // the kernels dereference these: memory of the device, or nothing is launched
        for (int c = 0; c < n_cols; ++c) {
            if (n_rows > 0 && !on_device(device, valid[(size_t)c])) return fail(LP_E_INVALID);
            if (cols[(size_t)c].form == LP_ARROW_MAP && !on_device(device, cols[(size_t)c].map->entry_off)) return fail(LP_E_INVALID);
        }
        hipStream_t s = (hipStream_t)stream;
        unsigned long long* d_count = (unsigned long long*)S.get(8 * (size_t)n_cols);
        if (!d_count) return fail(LP_E_NOMEM);
        hipEvent_t ev[2] = {nullptr, nullptr};
        const bool timed = pack_ms && hipEventCreate(&ev[0]) == hipSuccess && hipEventCreate(&ev[1]) == hipSuccess;
        auto done = [&](int rc) {
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
            return rc == LP_OK ? rc : fail(rc);
        };
        if (timed) hipEventRecord(ev[0], s);
        if (hipMemsetAsync(d_count, 0, 8 * (size_t)n_cols, s) != hipSuccess) return done(LP_E_DEVICE);
        for (int c0 = 0; n_rows > 0 && c0 < n_cols; c0 += ARROW_MAX_COLS) {
            ArrowValidArgs A{};
            const int nc = n_cols - c0 < ARROW_MAX_COLS ? n_cols - c0 : ARROW_MAX_COLS;
            for (int c = 0; c < nc; ++c) A.col[c] = {valid[(size_t)(c0 + c)], bitmap[(size_t)(c0 + c)], d_count + c0 + c};
            if (launch_arrow_validity(A, nc, n_rows, s) != 0) return done(LP_E_DEVICE);
        }
        for (int c = n_plain + n_dict; c < n_cols; ++c)
            if (launch_arrow_narrow32(cols[(size_t)c].map->entry_off, const_cast<int32_t*>(cols[(size_t)c].off32), n_rows + 1, s) != 0)
                return done(LP_E_DEVICE);
        if (timed) hipEventRecord(ev[1], s);
        // one read-back of all counters, one synchronise
        std::vector<unsigned long long> cnt((size_t)n_cols, 0);
        if (hipMemcpyAsync(cnt.data(), d_count, 8 * (size_t)n_cols, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return done(LP_E_DEVICE);
        for (int c = 0; c < n_cols; ++c) n_valid[(size_t)c] = (int64_t)cnt[(size_t)c];
        if (timed) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) *pack_ms = t;
            else (void)hipGetLastError();
        }
        done(LP_OK);
        S.drop(d_count);
    }
    // a column without nulls carries no bitmap
    for (int c = 0; c < n_cols; ++c) {
        arrow::Col& C = cols[(size_t)c];
        C.nulls = n_rows - n_valid[(size_t)c];
        if (C.nulls == 0 && bitmap[(size_t)c]) {
            S.drop(bitmap[(size_t)c]);
            bitmap[(size_t)c] = nullptr;
        }
        C.bitmap = bitmap[(size_t)c];
    }
    std::vector<arrow::Col> ordered;
    for (int k = 0; k < n_cols; ++k) ordered.push_back(cols[(size_t)(order ? order[k] : k)]);
    arrow::Shared* sh = new arrow::Shared;
    sh->free_buf = host ? free : hip_free_buf;
    for (void* p : S.bufs)
        if (p) sh->owned.push_back(p);
    if (owner) sh->owner = *owner;
    arrow::build_batch(n_rows, ordered, host, sh, schema_out, &array_out->array);
    array_out->device_id = host ? -1 : device;
    array_out->device_type = host ? ARROW_DEVICE_CPU : ARROW_DEVICE_ROCM;
    array_out->sync_event = nullptr;  // the stream is synchronised: the buffers are complete
    return LP_OK;
}

namespace {

// lp_arrow_to_host: the copy of one array and what hangs below it
struct HostCopy {
    arrow::Shared* sh;
    bool from_device;
    int err = LP_OK;
    bool fetch(void* dst, const void* src, size_t bytes) {
        if (bytes == 0) return true;
        if (!src) return (err = LP_E_INVALID, false);
        if (!from_device) memcpy(dst, src, bytes);
        else if (hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return (err = LP_E_DEVICE, false);
        return true;
    }
    const void* copy(const void* src, size_t bytes) {
        void* p = calloc((bytes + 64) & ~(size_t)63, 1);
        if (!p) return (err = LP_E_NOMEM, nullptr);
        sh->owned.push_back(p);
        return fetch(p, src, bytes) ? p : nullptr;
    }
};

void drop_built(std::vector<ArrowArray*>& kids) {
    for (ArrowArray* k : kids) {
        arrow::release_array(k);
        delete k;
    }
    kids.clear();
}

int copy_array(HostCopy& H, const ArrowSchema* s, const ArrowArray* in, ArrowArray* out) {
    if (!s || !in || !s->format || !in->release || in->offset != 0 || in->length < 0) return LP_E_INVALID;
    if (in->n_children != s->n_children || (in->dictionary != nullptr) != (s->dictionary != nullptr)) return LP_E_INVALID;
    const std::string f = s->format;
    const int64_t n = in->length;
    auto buf = [&](int k) { return in->buffers && k < in->n_buffers ? in->buffers[k] : nullptr; };
    const void* b[3] = {nullptr, nullptr, nullptr};
    int nb = 0;
    if (f == "l" || f == "g" || f == "i") {
        nb = 2;
        if (in->n_buffers != 2 || !(b[1] = H.copy(buf(1), (f == "i" ? 4 : 8) * (size_t)n))) return H.err ? H.err : LP_E_INVALID;
    } else if (f == "U" || f == "Z") {
        nb = 3;
        int64_t last = 0;
        if (in->n_buffers != 3 || !buf(1) || !H.fetch(&last, (const int64_t*)buf(1) + n, 8)) return H.err ? H.err : LP_E_INVALID;
        if (last < 0) return LP_E_INVALID;
        if (!(b[1] = H.copy(buf(1), 8 * ((size_t)n + 1))) || !(b[2] = H.copy(buf(2), (size_t)last))) return H.err;
    } else if (f == "+m") {
        nb = 2;
        if (in->n_buffers != 2 || in->n_children != 1 || !buf(1)) return LP_E_INVALID;
        if (!(b[1] = H.copy(buf(1), 4 * ((size_t)n + 1)))) return H.err;
    } else if (f == "+s") {
        nb = 1;
    } else {
        return LP_E_INVALID;
    }
    if (buf(0) && !(b[0] = H.copy(buf(0), arrow::bitmap_bytes(n)))) return H.err;
    std::vector<ArrowArray*> kids;
    for (int64_t k = 0; k < in->n_children; ++k) {
        ArrowArray* a = new ArrowArray{};
        const int rc = in->children && s->children ? copy_array(H, s->children[k], in->children[k], a) : LP_E_INVALID;
        if (rc != LP_OK) {
            delete a;
            drop_built(kids);
            return rc;
        }
        kids.push_back(a);
    }
    ArrowArray* d = nullptr;
    if (in->dictionary) {
        d = new ArrowArray{};
        const int rc = copy_array(H, s->dictionary, in->dictionary, d);
        if (rc != LP_OK) {
            delete d;
            drop_built(kids);
            return rc;
        }
    }
    arrow::make_array(out, H.sh, n, in->null_count, nb, b[0], b[1], b[2], std::move(kids), d);
    return LP_OK;
}

}  // namespace
}  // namespace lp

extern "C" {

int lp_arrow_from_tables(int device, void* stream, int64_t n_rows, const lp_table_col* plain,
                         const char* const* plain_names, int n_plain, const lp_table_dict_col* dict,
                         const char* const* dict_names, int n_dict, const lp_table_map_col* map,
                         const char* const* map_names, int n_map, const lp_arrow_owner* owner, ArrowSchema* schema_out,
                         ArrowDeviceArray* array_out) {
    try {
        return lp::arrow_wrap(device, stream, n_rows, plain, plain_names, n_plain, dict, dict_names, n_dict, map, map_names,
                              n_map, nullptr, owner, schema_out, array_out, nullptr);
    } catch (const std::bad_alloc&) {
        return LP_E_NOMEM;
    }
}

int lp_arrow_to_host(const ArrowSchema* schema, const ArrowDeviceArray* in, ArrowArray* out) {
    if (out) memset(out, 0, sizeof *out);
    if (!schema || !in || !out || !schema->release) return LP_E_INVALID;
    if (in->device_type != ARROW_DEVICE_CPU && in->device_type != ARROW_DEVICE_ROCM) return LP_E_INVALID;
    const bool from_device = in->device_type == ARROW_DEVICE_ROCM;
    if (from_device && hipSetDevice((int)in->device_id) != hipSuccess) return LP_E_DEVICE;
    try {
        lp::arrow::Shared* sh = new lp::arrow::Shared;
        sh->free_buf = free;
        sh->refs.fetch_add(1);  // this call's own, until the copy stands or fails
        lp::HostCopy H{sh, from_device};
        const int rc = lp::copy_array(H, schema, &in->array, out);
        lp::arrow::shared_unref(sh);  // (a failed copy: the last reference, its buffers go)
        if (rc != LP_OK) memset(out, 0, sizeof *out);
        return rc;
    } catch (const std::bad_alloc&) {
        return LP_E_NOMEM;
    }
}

}  // extern "C"
