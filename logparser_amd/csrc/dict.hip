// gfx950 kernels of the dictionary-encoded STRING columns: lp_result_table_dict
// on a device view (include/logparser_amd.h) -- Arrow dictionary<int32, utf8>,
// what a Hive / ORC / Parquet writer's dictionary string encoding takes: a
// 4-byte index per row and each distinct value once, in the order of first
// occurrence.  The column's plain bytes are never written.  Per column, after
// k_table_values (table.hip) left each row's validity, length and source word:
//
//   k_dict_insert  one lane per valid row: the 64-bit hash of its bytes
//                  (lp_dict.h) into an open-addressing table of row numbers --
//                  an empty slot is claimed by compare-and-swap, an occupied
//                  one compared (length, then bytes) against the row it
//                  holds: equal -> the smaller row stays (atomic min), else
//                  the next slot.  The row remembers its slot.
//   k_dict_mark    a row is its class's representative when its slot holds
//                  the row itself: the class's smallest row, its first occurrence
//   (scan)         the flags -> each representative's entry number, their count
//   k_dict_index   index[k] = the entry of the representative in row k's
//                  slot; the representatives' lines, in row order
//   (table.hip)    the dictionary's values are the STRING column of the
//                  representatives' lines: the row-list instances of
//                  k_table_values / k_table_chars, launched by the caller
//
// A row's bytes are read where k_table_values found them (TableArgs::srcw):
// from the input or the arena, or formatted again into registers (a long, a
// date, a month name, a binary IP: at most 20 bytes).  A column may deliver
// the same text in two representations (CLF2NUM's null -> 0L against a token
// "0"): the hash and the comparison work on the bytes' 8-byte words, the same
// for every representation.
#include <hip/hip_runtime.h>

#define LP_KERNEL_TU 1  // device column pointers are global-memory pointers (lp_program.h)

#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "lp_device.h"
#include "lp_dict.h"
#include "table_value.h"  // TVal, tvalue, row_view

namespace lp {

namespace {

constexpr int TB = 256;

// a row's value: n bytes at p (amp: a '&' first, counted in n), or (packed)
// in the little-endian words w0 w1 w2
struct DVal {
    uint32_t n = 0;
    bool packed = false, amp = false;
    const LP_G uint8_t* p = nullptr;
    uint64_t w0 = 0, w1 = 0, w2 = 0;
};

typedef uint64_t __attribute__((aligned(1))) u64_unaligned;  // a value starts at any byte

__device__ __forceinline__ void dv_put(DVal& v, uint32_t q, uint32_t c) {
    const uint64_t b = (uint64_t)(c & 0xFFu) << (8 * (q & 7u));
    if (q < 8) v.w0 |= b;
    else if (q < 16) v.w1 |= b;
    else v.w2 |= b;
}

__device__ __forceinline__ void dv_long(DVal& v, int64_t l) {
    uint64_t u = l < 0 ? 0 - (uint64_t)l : (uint64_t)l;
    uint32_t q = digits(l);
    v.packed = true;
    do {
        dv_put(v, --q, '0' + (uint32_t)(u % 10));
        u /= 10;
    } while (u);
    if (l < 0) dv_put(v, 0, '-');
}

// bytes [8j, 8j + 8) of the value, zero-padded past its end
__device__ __forceinline__ uint64_t dv_word(const DVal& v, uint32_t j) {
    if (v.packed) return j == 0 ? v.w0 : j == 1 ? v.w1 : j == 2 ? v.w2 : 0;
    const uint32_t o = 8 * j;
    if (!v.amp && o + 8 <= v.n) return *reinterpret_cast<const LP_G u64_unaligned*>(v.p + o);
    uint64_t x = 0;
    for (uint32_t t = 0; t < 8 && o + t < v.n; ++t) {
        const uint32_t at = o + t;
        const uint32_t b = v.amp ? (at == 0 ? (uint32_t)'&' : v.p[at - 1]) : v.p[at];
        x |= (uint64_t)b << (8 * t);
    }
    return x;
}

// valid row k's value, as k_table_chars finds it (a valid row's line is
// inside the batch: k_table_values checked it)
__device__ __forceinline__ DVal dict_value(const Program& P, const Columns& C, const TableArgs& T, const DictArgs& D,
                                           const uint8_t* buf, int64_t k) {
    DVal v;
    v.n = (uint32_t)D.len[k + 1];
    const uint64_t w = D.srcw[k];
    if ((w >> 62) == 0) {
        v.p = reinterpret_cast<const LP_G uint8_t*>((uintptr_t)(w & (SW_AMP - 1)));
        v.amp = (w & SW_AMP) != 0;
    } else if ((w >> 62) == 1) {
        dv_long(v, (int64_t)(w << 2) >> 2);
    } else {
        const TableCol& col = T.cols[0];
        const int64_t i = T.rows ? T.rows[k] : T.first + k;
        const LP_G uint8_t *line = nullptr, *region = nullptr;
        TVal t;
        if (row_view(P, C, buf, i, line, region)) {
            const int fmt = P.n_fmt > 1 ? (int)C.fmt_id[i] : 0;
            t = tvalue(P, C, T, col.src[fmt], i, line, region);
            if (t.kind == 0) t = tvalue(P, C, T, col.alt[fmt], i, line, region);  // the earlier delivery
        }
        if (t.kind == 2) {
            dv_long(v, t.l);
        } else if (t.kind == 3) {
            v.packed = true;
#pragma unroll
            for (uint32_t q = 0; q < 20; ++q)
                if (q < t.n) dv_put(v, q, (uint8_t)t.buf[q]);
        } else {
            v.p = t.p;
            v.amp = t.amp;
        }
    }
    return v;
}

__global__ __launch_bounds__(TB) void k_dict_insert(const DeviceArgs* __restrict__ args,
                                                    const TableArgs* __restrict__ targs, const DictArgs D,
                                                    const uint8_t* buf) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const TableArgs& T = *targs;
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= D.count) return;
    if (!D.valid[k]) {
        D.slot[k] = DICT_EMPTY;
        return;
    }
    const DVal a = dict_value(P, C, T, D, buf, k);
    const uint64_t h = dict_hash(a.n, [&](uint32_t j) { return dv_word(a, j); });
    // row r of an occupied slot: a row of this launch whose validity, length and
    // source word an earlier launch wrote
    auto same = [&](uint32_t r) {
        if ((uint32_t)D.len[(int64_t)r + 1] != a.n) return false;
        const DVal b = dict_value(P, C, T, D, buf, (int64_t)r);
        if (!a.packed && !b.packed && a.p == b.p && a.amp == b.amp) return true;
        for (uint32_t j = 0; 8 * j < a.n; ++j)
            if (dv_word(a, j) != dv_word(b, j)) return false;
        return true;
    };
    const uint32_t s = dict_insert<DictAtDevice>(D.slots, D.cap, dict_home(h, D.cap, D.hash_bits), (uint32_t)k, same);
    D.slot[k] = s;
    if (s == DICT_EMPTY) *D.fail = 1u;  // (every lane that runs out stores the same 1)
}

__global__ __launch_bounds__(TB) void k_dict_mark(const DictArgs D) {
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= D.count) return;
    uint32_t f = 0;
    if (D.valid[k]) {
        const uint32_t s = D.slot[k];
        f = s != DICT_EMPTY && D.slots[s] == (uint32_t)k ? 1u : 0u;
    }
    D.flag[k] = f;
}

// (rows: a generic pointer -- an address-space pointer among a kernel's own parameters would give the
// kernel one mangled name in the host pass and another in the device pass)
__global__ __launch_bounds__(TB) void k_dict_index(const DictArgs D, const int64_t* rows_arg, int64_t first) {
    const LP_G int64_t* rows = (const LP_G int64_t*)rows_arg;
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= D.count) return;
    int32_t e = 0;
    if (D.valid[k]) {
        const uint32_t s = D.slot[k];
        // rank: the flags' inclusive scan; a representative's entry is its rank - 1
        if (s != DICT_EMPTY) e = (int32_t)(D.rank[D.slots[s]] - 1u);
        if (D.flag[k]) D.reps[D.rank[k] - 1u] = rows ? rows[k] : first + k;
    }
    D.index[k] = e;
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
unsigned blocks_of(int64_t n) { return (unsigned)((n + TB - 1) / TB); }

}  // namespace

DictLayout dict_layout(int64_t count) {
    DictLayout L{};
    const size_t n = (size_t)(count > 0 ? count : 0);
    L.cap = dict_capacity(count);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += al256(bytes); return o; };
    // the table's scans run over the dictionary's rows (at most count); 64 KiB
    // more in case a shorter scan wants more temporary storage than a longer one
    L.table_bytes = table_srcw_offset(count) + 65536;
    L.table = take(L.table_bytes > 4 * (size_t)L.cap ? L.table_bytes : 4 * (size_t)L.cap);
    L.len = take(8 * (n + 1));
    L.srcw = take(8 * n);
    L.slot = take(4 * n);
    L.flag = take(4 * n);
    L.rank = take(4 * n);
    L.reps = take(8 * n);
    hipcub::DeviceScan::InclusiveSum(nullptr, L.tmp_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n);
    L.tmp = take(L.tmp_bytes);
    L.words = take(256);  // fail at 0, TableArgs::bad_row at 128
    L.total = at;
    return L;
}

void dict_bind(DictArgs& da, TableArgs& ta, const DictLayout& L, void* scratch) {
    char* b = (char*)scratch;
    // (a C-style cast: in the device pass the members are global-memory pointers)
    auto at = [&](auto& dst, size_t off) { dst = (std::remove_reference_t<decltype(dst)>)(b + off); };
    da.cap = L.cap;
    at(da.slots, L.table);
    at(da.len, L.len);
    at(da.srcw, L.srcw);
    at(da.slot, L.slot);
    at(da.flag, L.flag);
    at(da.rank, L.rank);
    at(da.reps, L.reps);
    at(da.fail, L.words);
    at(ta.cols[0].i64, L.len);
    at(ta.srcw, L.srcw);
    at(ta.bad_row, L.words + 128);
}

int launch_dict_insert(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const DictArgs& da,
                       const uint8_t* buf, hipStream_t s) {
    if (da.count <= 0 || da.count > 0x7FFFFFFF || da.cap < 2 * (uint64_t)da.count) return -1;
    // the table is reset on every call: every slot DICT_EMPTY
    if (hipMemsetAsync((void*)da.slots, 0xFF, 4 * (size_t)da.cap, s) != hipSuccess) return -1;
    if (hipMemsetAsync((void*)da.fail, 0, 4, s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_dict_insert, dim3(blocks_of(da.count)), dim3(TB), 0, s, d_args, d_targs, da, buf);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dict_rank(const DictArgs& da, const DictLayout& L, void* scratch, hipStream_t s, const uint32_t** total) {
    if (da.count <= 0 || da.count > 0x7FFFFFFF) return -1;  // the scan's item count is an int
    const int items = (int)da.count;
    hipLaunchKernelGGL(k_dict_mark, dim3(blocks_of(items)), dim3(TB), 0, s, da);
    size_t t = L.tmp_bytes;
    if (hipcub::DeviceScan::InclusiveSum((char*)scratch + L.tmp, t, (const uint32_t*)da.flag, (uint32_t*)da.rank, items, s) !=
        hipSuccess)
        return -1;
    *total = (const uint32_t*)da.rank + (da.count - 1);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_dict_index(const TableArgs& ta, const DictArgs& da, hipStream_t s) {
    if (da.count <= 0) return -1;
    hipLaunchKernelGGL(k_dict_index, dim3(blocks_of(da.count)), dim3(TB), 0, s, da, (const int64_t*)ta.rows, ta.first);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lp
