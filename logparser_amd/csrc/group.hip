// gfx950 kernels of lp_result_group on a device view (include/logparser_amd.h):
// GROUP BY over the rows of a parsed batch -- the groups of a key tuple in the
// order of first occurrence, each group's first line, every row's group, and
// COUNT / SUM / MIN / MAX of LONG measures per group.  No key or measure
// column is written: each value is derived where it is needed, as where.hip's
// predicate does.
//
//   k_group_insert  one lane per row: the row's key values (the pseudo-columns
//                   before the status test, then src, then alt), their tuple's
//                   64-bit hash (lp_group.h) stored per row, and lp_dict.h's
//                   insert into the table of row numbers; same(r) looks at
//                   row r's stored hash, then compares every key in full with
//                   both rows' values derived again
//   (dict.hip)      k_dict_mark, the rank scan and k_dict_index number the
//                   groups by first occurrence: group_of and the groups' lines
//   k_group_fill    every accumulator word's identity
//   k_group_agg     one lane per row: its group, each distinct measure's LONG
//                   value, and what the row gives each of the group's words
//                   (lp_group.h) -- privatised: into the block's copy in LDS,
//                   flushed at the block's end with one agent-scope atomic per
//                   touched (block, group, word); direct: the wave peels its
//                   leading groups (first active lane's group, the ballot of
//                   the lanes that share it, a wave reduction, one atomic by
//                   the leader) for a fixed number of rounds, the lanes left
//                   issue their own atomics
//   k_group_finish  value / valid of each (group, aggregate) out of the words
//
// The "value of (column, row)" step and the packed words of a formatted value
// restate where.hip's and dict.hip's: those units' kernels keep the code and
// the registers they had.
#include <hip/hip_runtime.h>

#define LP_KERNEL_TU 1  // device column pointers are global-memory pointers (lp_program.h)

#include "kernels_common.h"  // lane_id
#include "lp_group.h"
#include "table_value.h"  // TVal, tvalue_any, has_geo, row_line

namespace lp {

namespace {

constexpr int TB = 256;
constexpr int AGG_MAX_BLOCKS = 1024;  // k_group_agg's grid: four blocks per CU, each striding over the rows

typedef GroupAtDevice<__HIP_MEMORY_SCOPE_AGENT> AtGlobal;
typedef GroupAtDevice<__HIP_MEMORY_SCOPE_WORKGROUP> AtBlock;

// a row's line: what every column's value is derived from
struct RowCtx {
    int64_t i;
    uint32_t st;
    bool ok;  // status OK: the real columns have values
    int fmt;
    const LP_G uint8_t *line, *region;
};

__device__ __forceinline__ RowCtx row_ctx(const Program& P, const Columns& C, const uint8_t* buf, int64_t i) {
    RowCtx R;
    R.i = i;
    R.st = C.status[i];
    R.ok = R.st == ST_OK;
    R.line = R.region = nullptr;
    if (R.ok) {  // (row_view, the status known)
        R.line = (const LP_G uint8_t*)buf + C.line_off[i];
        R.region = P.has_phase2() ? C.arena + C.arena_base[i] : C.arena;
    }
    R.fmt = R.ok && P.n_fmt > 1 ? (int)C.fmt_id[i] : 0;
    return R;
}

// The value lp_result_table_rows would build for the row and the column (its
// kind 1 STRING / 2 LONG); false: null.  A LONG column's value is v.l (v.kind
// 2); a STRING column's is bytes at v.p (kind 1), a long whose decimal text it
// is (kind 2), or bytes in v.buf (kind 3).
template <bool EXT, bool GEO>
__device__ __forceinline__ bool col_value(const Program& P, const Columns& C, const TableArgs& T, const TableCol& col,
                                          const uint8_t* buf, const RowCtx& R, TVal& v) {
    bool valid = false;
    if constexpr (EXT) {
        // a pseudo-column: valid for every status
        const int32_t pk = col.src[0].kind;
        if (tc_pseudo(pk)) {
            if (pk == TC_LINE) {  // the parse kernels' line: wave_lines' end, crlf_len
                const uint64_t s0 = C.line_off[R.i], e0 = C.line_off[R.i + 1] - 1;
                const LP_G uint8_t* lp = (const LP_G uint8_t*)buf + s0;
                uint64_t n = e0 - s0;
                if (n > 0 && lp[n - 1] == '\r') --n;
                v.kind = 1;
                v.p = lp;
                v.n = (uint32_t)n;
            } else {
                v.kind = 2;
                v.l = pk == TC_OFFSET ? (int64_t)C.line_off[R.i] : pk == TC_LINENO ? T.first_line + R.i : (int64_t)R.st;
            }
            return true;
        }
    }
    // the later delivery, then (a value that is none for the column) the earlier
    for (int pass = 0; pass < 2 && R.ok && !valid; ++pass) {
        const TableSrc& sc = pass ? col.alt[R.fmt] : col.src[R.fmt];
        if (pass && sc.kind == TC_NONE) break;
        v = tvalue_any<GEO>(P, C, T, sc, R.i, R.line, R.region);
        valid = v.kind != 0;
        if (col.kind == 2) {  // LONG: parse_long of text; month names, dates: not numbers
            if (v.kind == 1) {
                int64_t x = 0;
                valid = parse_long(v.p, v.n, v.amp, x);
                v.kind = 2;
                v.l = x;
            } else if (v.kind == 3) {
                valid = false;
            }
        }
    }
    return valid;
}

// ---- a key's value as words (dict.hip's DVal, restated): n bytes at p (amp: a
// '&' first, counted in n), or (packed) in the little-endian words w0 w1 w2;
// a LONG key: l
struct GKey {
    bool null = true, packed = false, amp = false;
    uint32_t n = 0;
    const LP_G uint8_t* p = nullptr;
    uint64_t w0 = 0, w1 = 0, w2 = 0;
    int64_t l = 0;
};

typedef uint64_t __attribute__((aligned(1))) u64_unaligned;  // a value starts at any byte

__device__ __forceinline__ void gk_put(GKey& v, uint32_t q, uint32_t c) {
    const uint64_t b = (uint64_t)(c & 0xFFu) << (8 * (q & 7u));
    if (q < 8) v.w0 |= b;
    else if (q < 16) v.w1 |= b;
    else v.w2 |= b;
}

__device__ __forceinline__ void gk_long(GKey& v, int64_t l) {
    uint64_t u = l < 0 ? 0 - (uint64_t)l : (uint64_t)l;
    uint32_t q = digits(l);
    v.n = q;
    v.packed = true;
    do {
        gk_put(v, --q, '0' + (uint32_t)(u % 10));
        u /= 10;
    } while (u);
    if (l < 0) gk_put(v, 0, '-');
}

// bytes [8j, 8j + 8) of the value, zero-padded past its end
__device__ __forceinline__ uint64_t gk_word(const GKey& v, uint32_t j) {
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

template <bool EXT, bool GEO>
__device__ __forceinline__ GKey key_value(const Program& P, const Columns& C, const TableArgs& T, const TableCol& col,
                                          const uint8_t* buf, const RowCtx& R) {
    GKey k;
    TVal v;
    if (!col_value<EXT, GEO>(P, C, T, col, buf, R, v)) return k;
    k.null = false;
    if (col.kind == 2) {
        k.l = v.l;
    } else if (v.kind == 2) {  // a STRING taken from a long: its decimal text
        gk_long(k, v.l);
    } else if (v.kind == 3) {
        k.packed = true;
        k.n = v.n;
#pragma unroll
        for (uint32_t q = 0; q < 20; ++q)
            if (q < v.n) gk_put(k, q, (uint8_t)v.buf[q]);
    } else {
        k.n = v.n;
        k.p = v.p;
        k.amp = v.amp;
    }
    return k;
}

// both null, or both non-null and equal: by value (LONG), by bytes (STRING)
__device__ __forceinline__ bool key_equal(int32_t kind, const GKey& a, const GKey& b) {
    if (a.null || b.null) return a.null && b.null;
    if (kind == 2) return a.l == b.l;
    if (a.n != b.n) return false;
    if (!a.packed && !b.packed && a.p == b.p && a.amp == b.amp) return true;
    for (uint32_t j = 0; 8 * j < a.n; ++j)
        if (gk_word(a, j) != gk_word(b, j)) return false;
    return true;
}

template <bool EXT, bool GEO>
__global__ __launch_bounds__(TB) void k_group_insert(const DeviceArgs* __restrict__ args, const TableArgs* __restrict__ targs,
                                                     const GroupArgs G, const uint8_t* buf) {
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const TableArgs& T = *targs;
    const int64_t k = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (k >= G.count) return;
    int64_t i;
    if (!row_line(T.rows, T.first, T.n_lines, T.bad_row, k, i)) {  // (the call fails: LP_E_INVALID)
        G.valid[k] = 0;
        G.slot[k] = DICT_EMPTY;
        return;
    }
    G.valid[k] = 1;
    const RowCtx R = row_ctx(P, C, buf, i);
    uint64_t h = GROUP_SEED;
    for (int c = 0; c < G.n_keys; ++c) {
        const GKey a = key_value<EXT, GEO>(P, C, T, T.cols[c], buf, R);
        if (a.null) h = group_hash_null(h);
        else if (T.cols[c].kind == 2) h = group_hash_long(h, a.l);
        else h = group_hash_bytes(h, a.n, [&](uint32_t j) { return gk_word(a, j); });
    }
    h = group_hash_end(h, G.hash_bits);
    AtGlobal::store_hash(G.hash + k, h);
    // row r of an occupied slot: a row of this launch inside the batch (only such rows insert)
    auto same = [&](uint32_t r) {
        if (!group_hash_may_equal(AtGlobal::load_hash(G.hash + r), h)) return false;
        const int64_t ir = T.rows ? T.rows[r] : T.first + (int64_t)r;
        if (ir == i) return true;  // (a row list that repeats a line)
        const RowCtx Rr = row_ctx(P, C, buf, ir);
        for (int c = 0; c < G.n_keys; ++c) {
            const GKey a = key_value<EXT, GEO>(P, C, T, T.cols[c], buf, R);
            const GKey b = key_value<EXT, GEO>(P, C, T, T.cols[c], buf, Rr);
            if (!key_equal(T.cols[c].kind, a, b)) return false;
        }
        return true;
    };
    const uint32_t s = dict_insert<DictAtDevice>(G.slots, G.cap, dict_home(h, G.cap, G.hash_bits), (uint32_t)k, same);
    G.slot[k] = s;
    if (s == DICT_EMPTY) *G.fail = 1u;  // (every lane that runs out stores the same 1)
}

__global__ __launch_bounds__(TB) void k_group_fill(const GroupArgs G) {
    const int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x;
    const int W = G.A.n_words;
    if (x >= G.n_groups * W) return;
    G.acc[x] = group_identity(G.A.wkind[x % W]);
}

// the fold of `kind` over the lanes of `mask` (the others give the identity), in every lane
__device__ __forceinline__ int64_t wave_fold(int32_t kind, int64_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = group_merge(kind, v, (int64_t)__shfl_xor((long long)v, d));
    return v;
}

template <bool EXT, bool GEO, bool LDS>
__global__ __launch_bounds__(TB) void k_group_agg(const DeviceArgs* __restrict__ args, const TableArgs* __restrict__ targs,
                                                  const GroupArgs G, const uint8_t* buf) {
    extern __shared__ __attribute__((aligned(16))) int64_t lacc[];  // LDS: n_groups x words, the block's copy
    const Program& P = args->prog;
    const Columns& C = args->cols;
    const TableArgs& T = *targs;
    const GroupAccs& A = G.A;
    const int W = A.n_words;
    const int64_t total = LDS ? G.n_groups * W : 0;
    if constexpr (LDS) {
        for (int64_t x = threadIdx.x; x < total; x += TB) lacc[x] = group_identity(A.wkind[x % W]);
        __syncthreads();
    }
    // (the bound is the same for a block's lanes: every wave runs the same rounds, whole)
    for (int64_t k0 = (int64_t)blockIdx.x * TB; k0 < G.count; k0 += (int64_t)gridDim.x * TB) {
        const int64_t k = k0 + threadIdx.x;
        int64_t i = 0;
        // (a row outside the batch was refused before this launch; checked again, never dereferenced)
        const bool live = k < G.count && row_line(T.rows, T.first, T.n_lines, T.bad_row, k, i);
        const int64_t g = live ? (int64_t)G.group_of[k] : 0;
        // each distinct measure's LONG value, once
        int64_t val[GROUP_MAX_AGGS];
        uint32_t okm = 0;
#pragma unroll
        for (int m = 0; m < GROUP_MAX_AGGS; ++m) val[m] = 0;
        if (live && A.n_meas > 0) {
            const RowCtx R = row_ctx(P, C, buf, i);
#pragma unroll
            for (int m = 0; m < GROUP_MAX_AGGS; ++m) {
                if (m >= A.n_meas) break;
                TVal v;
                if (col_value<EXT, GEO>(P, C, T, T.cols[G.n_keys + m], buf, R, v)) {
                    okm |= 1u << m;
                    val[m] = v.l;
                }
            }
        }
        // what the row gives word w (its identity: nothing)
        auto contrib = [&](int w) {
            const int wm = A.wmeas[w];
            int64_t x = 0;
#pragma unroll
            for (int m = 0; m < GROUP_MAX_AGGS; ++m)
                if (m == wm) x = val[m];
            const int32_t kind = A.wkind[w];
            return live ? group_contrib(kind, wm >= 0 && ((okm >> wm) & 1u), x) : group_identity(kind);
        };
        if constexpr (LDS) {
            if (live)
                for (int w = 0; w < W; ++w) group_fold<AtBlock>(lacc + g * W + w, A.wkind[w], contrib(w));
        } else {
            // the wave's leading groups, one atomic each per word; never to exhaustion
            // (cand: the lanes not yet looked at; mine: those that still owe their own atomics.  A
            // leading group of one row costs its round two ballots and stays with its lane: a wave of
            // 64 distinct groups runs G.peel such rounds, no reduction)
            bool cand = live, mine = live;
            for (int round = 0; round < G.peel; ++round) {
                const uint64_t left = __ballot(cand);
                if (left == 0) break;
                const int64_t gl = __shfl((long long)g, (int)__builtin_ctzll(left));  // (readfirstlane of an active lane)
                const bool in = cand && g == gl;
                const uint64_t share = __ballot(in);
                cand = cand && !in;
                if (__builtin_popcountll(share) < 2) continue;
                const bool leader = in && (int)__builtin_ctzll(share) == (int)lane_id();
                for (int w = 0; w < W; ++w) {
                    const int32_t kind = A.wkind[w];
                    const int64_t v = wave_fold(kind, in ? contrib(w) : group_identity(kind));
                    if (leader) group_fold<AtGlobal>(G.acc + gl * W + w, kind, v);
                }
                mine = mine && !in;
            }
            if (mine)
                for (int w = 0; w < W; ++w) group_fold<AtGlobal>(G.acc + g * W + w, A.wkind[w], contrib(w));
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int64_t x = threadIdx.x; x < total; x += TB) group_fold<AtGlobal>(G.acc + x, A.wkind[x % W], lacc[x]);
    }
}

__global__ __launch_bounds__(TB) void k_group_finish(const GroupArgs G, const GroupOut O) {
    const int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x;
    const int n = G.A.n_aggs;
    if (x >= O.groups * n) return;
    const int64_t g = x / n;
    const int a = (int)(x % n);
    const LP_G int64_t* w = G.acc + g * G.A.n_words;
    const bool valid = G.A.op[a] <= GA_COUNT || w[1 + G.A.meas[a]] != 0;
    O.value[a][g] = valid ? w[G.A.word[a]] : 0;
    O.valid[a][g] = valid ? 1 : 0;
}

// a pseudo-column among the keys and measures (the same for every LogFormat)
bool has_pseudo(const TableArgs& ta) {
    for (int c = 0; c < ta.n_cols; ++c)
        if (tc_pseudo(ta.cols[c].src[0].kind)) return true;
    return false;
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
unsigned blocks_of(int64_t n) { return (unsigned)((n + TB - 1) / TB); }

}  // namespace

GroupLayout group_layout(int64_t count) {
    GroupLayout L{};
    const size_t n = (size_t)(count > 0 ? count : 0);
    L.cap = dict_capacity(count);
    const DictLayout D = dict_layout(count);  // (the rank scan's temporaries: their size)
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += al256(bytes); return o; };
    L.slots = take(4 * (size_t)L.cap);
    L.hash = take(8 * n);
    L.slot = take(4 * n);
    L.flag = take(4 * n);
    L.rank = take(4 * n);
    L.reps = take(8 * n);
    L.valid = take(n);
    L.group_of = take(4 * n);
    L.d.tmp_bytes = D.tmp_bytes;
    L.d.tmp = take(D.tmp_bytes);
    L.words = take(256);  // fail at 0, TableArgs::bad_row at 128
    L.total = at;
    return L;
}

void group_bind(GroupArgs& ga, DictArgs& da, TableArgs& ta, const GroupLayout& L, void* scratch, int32_t* group_of) {
    char* b = (char*)scratch;
    // (a C-style cast: in the device pass the members are global-memory pointers)
    auto at = [&](auto& dst, size_t off) { dst = (std::remove_reference_t<decltype(dst)>)(b + off); };
    ga.cap = da.cap = L.cap;
    at(ga.slots, L.slots);
    at(ga.hash, L.hash);
    at(ga.slot, L.slot);
    at(ga.valid, L.valid);
    at(ga.fail, L.words);
    at(da.slots, L.slots);
    at(da.slot, L.slot);
    at(da.valid, L.valid);
    at(da.flag, L.flag);
    at(da.rank, L.rank);
    at(da.reps, L.reps);
    at(da.fail, L.words);
    if (group_of) da.index = (decltype(da.index))group_of;
    else at(da.index, L.group_of);
    ga.group_of = (decltype(ga.group_of))da.index;
    at(ta.bad_row, L.words + 128);
}

int launch_group_insert(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const GroupArgs& ga,
                        const uint8_t* buf, hipStream_t s) {
    if (ga.count <= 0 || ga.count > 0x7FFFFFFF || ga.cap < 2 * (uint64_t)ga.count || ga.n_keys < 0 ||
        ga.n_keys > GROUP_MAX_KEYS)
        return -1;
    // reset on every call: every slot DICT_EMPTY, every stored hash 0 (not seen), the two flag words
    if (hipMemsetAsync((void*)ga.slots, 0xFF, 4 * (size_t)ga.cap, s) != hipSuccess) return -1;
    if (hipMemsetAsync((void*)ga.hash, 0, 8 * (size_t)ga.count, s) != hipSuccess) return -1;
    if (hipMemsetAsync((void*)ga.fail, 0, 256, s) != hipSuccess) return -1;
    const dim3 grid(blocks_of(ga.count)), tb(TB);
    const bool ext = has_pseudo(ta), geo = has_geo(ta);
    if (ext && geo) hipLaunchKernelGGL((k_group_insert<true, true>), grid, tb, 0, s, d_args, d_targs, ga, buf);
    else if (ext) hipLaunchKernelGGL((k_group_insert<true, false>), grid, tb, 0, s, d_args, d_targs, ga, buf);
    else if (geo) hipLaunchKernelGGL((k_group_insert<false, true>), grid, tb, 0, s, d_args, d_targs, ga, buf);
    else hipLaunchKernelGGL((k_group_insert<false, false>), grid, tb, 0, s, d_args, d_targs, ga, buf);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_group_agg(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const GroupArgs& ga,
                     const uint8_t* buf, int64_t lds_words, hipStream_t s, bool* privatised) {
    const int W = ga.A.n_words;
    if (ga.count <= 0 || ga.n_groups <= 0 || ga.n_groups > ga.count || W < 1 || W > GROUP_MAX_WORDS || !ga.acc ||
        !ga.group_of || ga.peel < 0 || ga.peel > GROUP_PEEL_MAX || ga.A.n_meas < 0 || ga.A.n_meas > GROUP_MAX_AGGS)
        return -1;
    if (lds_words > GROUP_LDS_WORDS_MAX) lds_words = GROUP_LDS_WORDS_MAX;
    const bool lds = group_privatised(ga.n_groups, W, lds_words);
    if (privatised) *privatised = lds;
    hipLaunchKernelGGL(k_group_fill, dim3(blocks_of(ga.n_groups * W)), dim3(TB), 0, s, ga);
    const unsigned want = blocks_of(ga.count);
    const dim3 grid(want < (unsigned)AGG_MAX_BLOCKS ? want : (unsigned)AGG_MAX_BLOCKS), tb(TB);
    const size_t shm = lds ? 8 * (size_t)(ga.n_groups * W) : 0;
    const bool ext = has_pseudo(ta), geo = has_geo(ta);
    auto go = [&](auto e, auto g) {
        if (lds) hipLaunchKernelGGL((k_group_agg<e.value, g.value, true>), grid, tb, shm, s, d_args, d_targs, ga, buf);
        else hipLaunchKernelGGL((k_group_agg<e.value, g.value, false>), grid, tb, 0, s, d_args, d_targs, ga, buf);
    };
    if (ext && geo) go(std::true_type{}, std::true_type{});
    else if (ext) go(std::true_type{}, std::false_type{});
    else if (geo) go(std::false_type{}, std::true_type{});
    else go(std::false_type{}, std::false_type{});
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_group_finish(const GroupArgs& ga, const GroupOut& go, hipStream_t s) {
    if (go.groups <= 0 || ga.A.n_aggs <= 0) return 0;
    hipLaunchKernelGGL(k_group_finish, dim3(blocks_of(go.groups * ga.A.n_aggs)), dim3(TB), 0, s, ga, go);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace lp
