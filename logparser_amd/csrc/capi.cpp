// C-ABI of the logparser_amd engine (include/logparser_amd.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <cmath>
#include <regex>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/logparser_amd.h"
#include "kernels.h"
#include "lp_arrow.h"
#include "lp_fixed.h"
#include "lp_pred.h"
#include "plan.h"

#if defined(LP_PROFILE)
// profiling build: copy out (and clear) the per-wave timestamps of the parse
// and URI kernels (PROF_WAVES x PROF_POINTS u64; the two kernel translation
// units mark disjoint points)
extern "C" int lp_profile_read(unsigned long long* out, int n) {
    if (n < lp::PROF_WAVES * lp::PROF_POINTS) return -1;
    std::vector<unsigned long long> u((size_t)lp::PROF_WAVES * lp::PROF_POINTS);
    if (lp::prof_read_parse(out) != 0 || lp::prof_read_uri(u.data()) != 0) return -1;
    for (size_t k = 0; k < u.size(); ++k) out[k] += u[k];
    lp::prof_clear_parse();
    lp::prof_clear_uri();
    return 0;
}
#endif

static_assert(LP_ARENA_SHARDS == lp::ARENA_SHARDS, "arena shard count of the ABI and the kernels");

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool ensure(size_t n) {
        if (n <= cap && p) return true;
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
        if (n == 0) n = 256;
        if (hipMalloc(&p, n) != hipSuccess) return false;
        cap = n;
        return true;
    }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T* as(size_t off = 0) const { return reinterpret_cast<T*>((char*)p + off); }
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// One SoA column of the program: its ABI name, stage index, element size and
// the Columns field that points at it.
struct ColSpec {
    const char* name;
    int index;
    int esz;
    void** field;
    int uri;  // written by the URI kernels (1) or the parse kernels (0): lp_last_bytes' per-kernel split
};

// The host tables' worker split: [0, count) in T chunks of per rows, the
// trailing ones empty when T does not divide count or exceeds it; chunk t is
// [at[t], at[t + 1]).
struct Chunks {
    int T;
    std::vector<int64_t> at;
    Chunks(int64_t count, int threads) : T(std::max(1, std::min(threads, 64))), at((size_t)T + 1) {
        const int64_t per = (count + T - 1) / T;
        for (int t = 0; t <= T; ++t) at[(size_t)t] = std::min(count, t * per);
    }
    // fn(t, a, b) for every chunk, one thread each (chunk 0 on the caller's)
    template <class F>
    void run(F fn) const {
        std::vector<std::thread> pool;
        for (int t = 1; t < T; ++t) pool.emplace_back([&, t] { fn(t, at[(size_t)t], at[(size_t)t + 1]); });
        fn(0, at[0], at[1]);
        for (auto& th : pool) th.join();
    }
};

// HIP-event times of a device call's phases, over the handle's one pool of
// table events (a handle's calls are serialised on its stream).  Asking HIP for
// the time between events of which one was not recorded in this call leaves
// hipErrorInvalidHandle behind, which the next launch's hipGetLastError takes
// for its own (an empty table once failed the next lp_parse_batch that way):
// elapsed() answers 0 for those without asking.
struct PhaseTimer {
    hipEvent_t* ev;
    hipStream_t s;
    bool on[6] = {false, false, false, false, false, false};
    void mark(int k) {
        hipEventRecord(ev[k], s);
        on[k] = true;
    }
    // event k for a launcher that records it itself, if it will
    hipEvent_t lend(int k, bool recorded) {
        on[k] = recorded;
        return ev[k];
    }
    float elapsed(int a, int b) const {
        float t = 0;
        if (on[a] && on[b]) hipEventElapsedTime(&t, ev[a], ev[b]);
        return t;
    }
};

// one total read back on the stream (the caller synchronises before it looks)
template <class V>
bool read_back(hipStream_t s, V* dst, const void* src) {
    return hipMemcpyAsync(dst, src, sizeof(V), hipMemcpyDeviceToHost, s) == hipSuccess;
}

// where each family's phases start in lp_handle::tms (lp_last_timing index - 5)
enum { TMS_TABLE = 0, TMS_MAP = 3, TMS_SELECT = 6, TMS_DICT = 7, TMS_ARROW = 11, TMS_WHERE = 12, TMS_GROUP = 14 };

}  // namespace

struct lp_handle {
    lp::Plan plan;
    int compile_status = LP_OK;
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf input, chunk, line_off, cols, arena, meta, waves, args, route, ovf, hist;
    DevBuf cstate;  // chunked parse: look-back words, per-chunk counts, queued lines
    DevBuf targs, tscratch;  // device table (lp_result_table on a device view)
    DevBuf gacc;             // lp_result_group's accumulator words (sized once the groups are counted)
    // the GeoIP stages' images on this handle's device (lp_geoip.h): a tree per database, a
    // field table and its byte pool per stage; uploaded at compile time, released by lp_free
    DevBuf geo_tree[lp::N_GEODB], geo_fields[lp::MAX_VAL], geo_pool[lp::MAX_VAL];
    lp::DeviceArgs host_args{};
    lp::Columns C{};
    std::vector<ColSpec> specs;
    std::vector<lp_column> dev_cols;
    // the batch (valid once lp_parse_batch succeeded)
    bool valid = false, pending = false;
    int64_t n_lines = 0;
    uint64_t nbytes = 0;
    const uint8_t* d_buf = nullptr;
    // capacities of the column and arena buffers, and what sizes the next batch
    int64_t cap_lines = 0;
    uint64_t shard_cap = 0;
    int64_t reserve_lines = 0;
    uint64_t reserve_arena = 0;
    double mean_line = 0;          // input bytes per line of the last batch
    double arena_per_line = 0;     // arena bytes (largest shard x shards) per line of the last batch
    bool force_direct = false;
    int max_retries = 3;           // re-runs of a batch whose estimates were short (LP_OPT_MAX_RETRIES)
    uint64_t arena_first = 0;      // LP_OPT_ARENA_BYTES: exact arena of a batch's first run (tests)
    uint64_t arena_ovf = 0;        // arena overflow events of the last batch's final run (its lines FALLBACK)
    int64_t first_line = 0;        // global number of the last batch's first line
    int64_t next_line = 0;         // ... of the next batch's (lp_parse_batch continues the numbering)
    hipEvent_t ev[7]{};  // batch start, index done, parse start, batch end, parse kernels done, k_geoip_lines start / end
    float geo_ms = 0;    // k_geoip_lines of the last batch (lp_last_timing [17])
    hipEvent_t tev[6]{}; // the device table calls' phase events (PhaseTimer): one pool, the calls are serialised
    // lp_last_timing [5..16], each family's last successful device call: the table's values / scans /
    // bytes phases; the map columns' count / entries / fill phases, summed over the columns;
    // lp_result_select's passes and scan; the dictionary columns' four phases, summed over the columns;
    // [16] lp_result_arrow's packaging kernels; ([17]: geo_ms;) [18..19] lp_result_select_where's
    // predicate kernel and compaction; [20..22] lp_result_group's insert, numbering and aggregation
    float tms[17]{};
    int dict_hash_bits = 0;  // LP_OPT_DICT_HASH_BITS (tests: 0 = the whole hash)
    int group_lds_words = 0; // LP_OPT_GROUP_LDS_WORDS (0: lp_group.h GROUP_LDS_WORDS, -1: none)
    int group_peel = 0;      // LP_OPT_GROUP_PEEL (0: lp_group.h GROUP_PEEL_ROUNDS, -1: none)
    bool have_events = false;
    uint64_t counters[4]{};
    uint32_t chunk_lines = 0;      // LP_OPT_CHUNK_LINES (0: the kernel's default)
    int32_t chunk_wait = 0;        // LP_OPT_CHUNK_WAIT (tests: 0 default, < 0 defer every chunk not yet reached)
    bool fixed_shape = true;       // LP_OPT_FIXED_SHAPE: the chunk kernel's fixed-shape instances (lp_fixed.h)
    uint64_t ovf_lines = 0;        // lines of the last batch the chunk kernel queued for k_parse_ovf_lines
    uint64_t uri_ovf_waves = 0;    // waves of the last batch whose URI stages ran in k_uri_overflow
    uint64_t deferred = 0;         // chunks of the last batch parsed by the deferred pass (normally 0)
    uint64_t dfs_lines = 0;        // lines of the last batch the chunk kernel queued for the backtracking DFS
    uint64_t walk_lines = 0;       // lines of the last batch whose first leaf took the element walk in a fixed-shape instance
    uint64_t uri_fix_lines = 0;    // lines of the last batch whose URI stages were redone with the repair on (uri_redo_line)
    uint64_t shard_top[LP_ARENA_SHARDS]{};
    lp::ParseLaunch last_launch{};  // the last enqueue's launch parameters (diagnostics)
    uint64_t arena_written = 0;
    uint64_t uri_src_bytes = 0;  // URI source bytes the URI kernels read (meta counters[5])
    int retries = 0;
    float ms[5]{};
    // host copy for lp_line_record_json / lp_line_status
    bool host_valid = false;
    std::vector<uint8_t> hostbuf;
    lp_result host_res{};
    lp::ResultView view;
    // HttpdLogFormatDissector's active format, carried from batch to batch
    // like the reference parser's (format 0 before the first line)
    uint32_t fmt_state = 0;
};

namespace {

// column capacity for n (expected) lines: 25 % more for the next batches of
// a stream, at most 4 M lines more (a huge batch keeps its footprint close to
// its size; a larger next batch re-runs once with exact capacity)
int64_t headroom(int64_t n) { return n + std::min<int64_t>(n / 4, 1 << 22) + 1024; }

void set_err(char* err, size_t errlen, const std::string& s) {
    if (err && errlen) snprintf(err, errlen, "%s", s.c_str());
}

// The program's SoA columns, in layout order.
void build_specs(lp_handle* h) {
    const lp::Program& P = h->plan.program();
    lp::Columns& C = h->C;
    auto& v = h->specs;
    v.clear();
    int uri = 0;
    auto add = [&](const char* nm, int idx, int esz, void* field) { v.push_back({nm, idx, esz, (void**)field, uri}); };
    add("status", 0, 1, &C.status);
    for (int k = 0; k < P.n_tok; ++k) add("tok_span", k, 4, &C.tok_span[k]);
    add("tok_flags", 0, 4, &C.tok_flags);
    add("hist", 0, 4, &C.hist);
    for (int t = 0; t < P.n_time; ++t) {
        add("t_epoch", t, 8, &C.t_epoch[t]);
        add("t_local", t, 8, &C.t_local[t]);
        add("t_utc", t, 8, &C.t_utc[t]);
        if (P.time[t].kind == lp::TK_STRF) add("t_nano", t, 4, &C.t_nano[t]);  // only strftime has fractions
    }
    for (int k = 0; k < P.n_secms; ++k) add("sm_ms", k, 8, &C.sm_ms[k]);
    for (int k = 0; k < P.n_binip; ++k) add("bip", k, 4, &C.bip[k]);
    for (int k = 0; k < P.n_val; ++k)
        if (P.val[k].kind == lp::VK_GEOIP) add("geo", k, 4, &C.geo[k]);  // (k_geoip_lines': neither kernel family's bytes)
    for (int f = 0; f < P.n_fl; ++f) {
        add("fl_kind", f, 4, &C.fl_kind[f]);
        add("fl_method", f, 4, &C.fl_method[f]);
        add("fl_uri", f, 4, &C.fl_uri[f]);
        add("fl_proto", f, 4, &C.fl_proto[f]);
    }
    uri = 1;  // the URI kernels' columns
    for (int u = 0; u < P.n_uri; ++u) {
        add("u_flags", u, 4, &C.u_flags[u]);
        add("u_scheme", u, 8, &C.u_scheme[u]);
        add("u_host", u, 8, &C.u_host[u]);
        add("u_port", u, 4, &C.u_port[u]);
        add("u_path", u, 8, &C.u_path[u]);
        add("u_query", u, 8, &C.u_query[u]);
        add("u_frag", u, 8, &C.u_frag[u]);
    }
    for (int q = 0; q < P.n_query; ++q) {
        add("q_count", q, 4, &C.q_count[q]);
        add("q_params", q, 8, &C.q_params[q]);
    }
    for (int j = 0; j < P.n_list; ++j) {
        add("l_count", j, 4, &C.l_count[j]);
        add("l_tab", j, 8, &C.l_tab[j]);
    }
    for (int j = 0; j < P.n_pair; ++j) {
        add("p_count", j, 4, &C.p_count[j]);
        add("p_tab", j, 8, &C.p_tab[j]);
    }
    add("arena_base", 0, 8, &C.arena_base);
    uri = 0;
    if (P.n_fmt > 1) {
        add("fmt_match", 0, 2, &C.fmt_match);
        add("fmt_id", 0, 1, &C.fmt_id);
    }
}

// column descriptors for columns of `rows` rows
std::vector<lp_column> layout(const std::vector<ColSpec>& specs, int64_t rows, uint64_t* total) {
    std::vector<lp_column> out;
    uint64_t off = 0;
    for (const auto& c : specs) {
        lp_column d{};
        snprintf(d.name, sizeof d.name, "%s", c.name);
        d.index = c.index;
        d.elem_size = c.esz;
        d.offset = off;
        out.push_back(d);
        off += align256((size_t)c.esz * (size_t)(rows > 0 ? rows : 1));
    }
    *total = off;
    return out;
}

// Columns for cap lines in one allocation.
bool alloc_columns(lp_handle* h, int64_t cap) {
    uint64_t total = 0;
    h->dev_cols = layout(h->specs, cap, &total);
    if (!h->cols.ensure(total)) return false;
    for (size_t k = 0; k < h->specs.size(); ++k) *h->specs[k].field = h->cols.as<char>(h->dev_cols[k].offset);
    return true;
}

// A view of a result (device or host copy) for the replay.
void make_view(lp_handle* h, const lp_result& r, lp::ResultView& V) {
    V = lp::ResultView{};
    V.n = r.n_lines;
    V.line_off = r.line_off;
    V.input = r.input;
    V.arena = r.arena;
    V.shard_cap = r.shard_cap;
    for (int s = 0; s < LP_ARENA_SHARDS; ++s) V.shard_off[s] = r.shard_off[s];
    for (int k = 0; k < r.n_columns; ++k) {
        const lp_column& c = r.column[k];
        const void* p = r.columns + c.offset;
        const std::string nm = c.name;
        const int i = c.index;
        if (nm == "status") V.status = (const uint8_t*)p;
        else if (nm == "tok_span") V.tok_span[i] = (const uint32_t*)p;
        else if (nm == "tok_flags") V.tok_flags = (const uint32_t*)p;
        else if (nm == "t_epoch") V.t_epoch[i] = (const int64_t*)p;
        else if (nm == "t_local") V.t_local[i] = (const uint64_t*)p;
        else if (nm == "t_utc") V.t_utc[i] = (const uint64_t*)p;
        else if (nm == "t_nano") V.t_nano[i] = (const uint32_t*)p;
        else if (nm == "fl_kind") V.fl_kind[i] = (const uint32_t*)p;
        else if (nm == "fl_method") V.fl_method[i] = (const uint32_t*)p;
        else if (nm == "fl_uri") V.fl_uri[i] = (const uint32_t*)p;
        else if (nm == "fl_proto") V.fl_proto[i] = (const uint32_t*)p;
        else if (nm == "u_flags") V.u_flags[i] = (const uint32_t*)p;
        else if (nm == "u_scheme") V.u_scheme[i] = (const uint64_t*)p;
        else if (nm == "u_host") V.u_host[i] = (const uint64_t*)p;
        else if (nm == "u_port") V.u_port[i] = (const int32_t*)p;
        else if (nm == "u_path") V.u_path[i] = (const uint64_t*)p;
        else if (nm == "u_query") V.u_query[i] = (const uint64_t*)p;
        else if (nm == "u_frag") V.u_frag[i] = (const uint64_t*)p;
        else if (nm == "q_count") V.q_count[i] = (const uint32_t*)p;
        else if (nm == "q_params") V.q_params[i] = (const uint64_t*)p;
        else if (nm == "arena_base") V.arena_base = (const uint64_t*)p;
        else if (nm == "sm_ms") V.sm_ms[i] = (const int64_t*)p;
        else if (nm == "l_count") V.l_count[i] = (const uint32_t*)p;
        else if (nm == "l_tab") V.l_tab[i] = (const uint64_t*)p;
        else if (nm == "bip") V.bip[i] = (const uint32_t*)p;
        else if (nm == "geo") V.geo[i] = (const uint32_t*)p;
        else if (nm == "p_count") V.p_count[i] = (const uint32_t*)p;
        else if (nm == "p_tab") V.p_tab[i] = (const uint64_t*)p;
        else if (nm == "fmt_id") V.fmt_id = (const uint8_t*)p;
    }
    if (!V.arena) V.arena_base = nullptr;
}

// The GeoIP stages' images to the handle's device, their pointers into h->C
// (copied into every batch's DeviceArgs): one tree per database, a field
// table and pool per stage.
bool upload_geo(lp_handle* h) {
    const lp::Program& P = h->plan.program();
    auto put = [](DevBuf& b, const void* src, size_t bytes) {
        if (!b.ensure(bytes + 16)) return false;
        return bytes == 0 || hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    for (int k = 0; k < P.n_val; ++k) {
        if (P.val[k].kind != lp::VK_GEOIP) continue;
        const lp::GeoImage& G = h->plan.geo_image(k);
        DevBuf& T = h->geo_tree[P.val[k].src_qname];
        if (!T.p && !put(T, G.tree->data(), 8 * G.tree->size())) return false;
        if (!put(h->geo_fields[k], G.fields.data(), sizeof(lp::GeoField) * G.fields.size())) return false;
        if (!put(h->geo_pool[k], G.pool.data(), G.pool.size())) return false;
        h->C.geo_tree[k] = T.as<uint64_t>();
        h->C.geo_fields[k] = h->geo_fields[k].as<uint64_t>();
        h->C.geo_pool[k] = h->geo_pool[k].as<uint8_t>();
        h->C.geo_records[k] = G.n_records;
    }
    return true;
}

// Enqueue the whole batch (index, routing, parse) with the current
// capacities.  sync_count: count the lines first and size the buffers from
// the exact count (the handle has no estimate yet).
// One LogFormat of the Apache common / combined family: literals, [^\s]*,
// the number kinds, .* / .*? and the %t time stamp, Apache time stages only,
// no cookie / Set-Cookie guards, SECOND_MILLIS or BinaryIP stages (the parse
// kernel's SIMPLE instance leaves the other kinds and stages out).
bool simple_program(const lp::Program& P) {
    if (P.n_fmt != 1 || P.n_secms || P.n_binip || P.guard_pct[0] || P.guard_setc[0]) return false;
    for (int t = 0; t < P.n_time; ++t)
        if (P.time[t].kind != lp::TK_APACHE) return false;
    for (int i = 0; i < P.n_elems; ++i) {
        switch (lp::load_elem(P.elems + i).kind) {
        case lp::EK_LIT: case lp::EK_NOSPACE: case lp::EK_NUMBER: case lp::EK_CLFNUMBER: case lp::EK_HEXNUMBER:
        case lp::EK_CLFHEXNUMBER: case lp::EK_NONZERO: case lp::EK_ANY_GREEDY: case lp::EK_ANY_LAZY:
        case lp::EK_TIME_US: break;
        default: return false;
        }
    }
    return true;
}

// The fixed shape (lp_fixed.h) whose chunk kernel instance parses P: only
// when every field that instance holds as a constant equals P's, field by
// field (fixed_shape_of), and its lines are in LDS.  Near-miss formats,
// requested-field subsets that change the capture slots or stage lists,
// several LogFormats and LP_OPT_FORCE_DIRECT get FS_NONE: the instances per
// program class.
int fixed_shape_program(const lp::Program& P, bool force_direct) {
    if (force_direct || !simple_program(P)) return lp::FS_NONE;
    return lp::fixed_shape_of(P);
}

int enqueue(lp_handle* h, bool sync_count) {
    hipStream_t s = h->stream;
    const uint64_t nbytes = h->nbytes;
    const lp::Program& P = h->plan.program();
    const int64_t nc = lp::count_chunks(nbytes);
    const size_t cbytes = align256(sizeof(uint64_t) * (size_t)(nc + 2));
    if (!h->chunk.ensure(cbytes + 2 * (size_t)lp::nlmask_words(nbytes))) return LP_E_NOMEM;
    if (!h->meta.ensure(sizeof(lp::Meta))) return LP_E_NOMEM;
    uint64_t* d_chunk = h->chunk.as<uint64_t>();
    uint16_t* d_nlmask = h->chunk.as<uint16_t>(cbytes);
    lp::Meta* d_meta = h->meta.as<lp::Meta>();
    if (hipMemsetAsync(d_meta, 0, sizeof(lp::Meta), s) != hipSuccess) return LP_E_DEVICE;
    hipEventRecord(h->ev[0], s);
    int64_t cap = h->cap_lines;
    // a device program: the parse kernel finds the lines itself
    // (k_parse_chunks); any other needs the line index built here
    const bool device = h->plan.device_ok();
    if (sync_count && device) {
        // first batch of a handle: the line length of an 8 MiB
        // prefix sizes the columns (no pass over the whole input; a short
        // estimate sets cap_ovf and finish() re-runs with the exact count)
        const uint64_t pre = std::min<uint64_t>(nbytes, 8ull << 20);
        if (!h->line_off.ensure(16)) return LP_E_NOMEM;
        if (lp::launch_count(h->d_buf, pre, d_chunk, d_nlmask, h->line_off.as<uint64_t>(), -1, d_meta, s) != 0)
            return LP_E_DEVICE;
        unsigned long long n = 0;
        if (hipMemcpyAsync(&n, &d_meta->n_lines, sizeof n, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess || hipMemsetAsync(d_meta, 0, sizeof(lp::Meta), s) != hipSuccess)
            return LP_E_DEVICE;
        const double mean = n ? (double)pre / (double)n : (double)std::max<uint64_t>(pre, 1);
        cap = std::max<int64_t>(headroom((int64_t)((double)nbytes / mean * 1.02)), h->reserve_lines);
        h->mean_line = mean;  // sizes this batch's LDS windows
    } else if (sync_count) {
        // first batch of a handle whose program is not on the device: the exact line count sizes the columns
        if (!h->line_off.ensure(16)) return LP_E_NOMEM;
        if (lp::launch_count(h->d_buf, nbytes, d_chunk, d_nlmask, h->line_off.as<uint64_t>(), -1, d_meta, s) != 0)
            return LP_E_DEVICE;
        unsigned long long n = 0;
        if (hipMemcpyAsync(&n, &d_meta->n_lines, sizeof n, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return LP_E_DEVICE;
        // headroom for the next batches of the stream (sized like the estimate below)
        cap = std::max<int64_t>(headroom((int64_t)n), h->reserve_lines);
        if (n) h->mean_line = (double)nbytes / (double)n;  // sizes this batch's LDS windows
    } else if (!device) {
        if (!h->line_off.ensure(sizeof(uint64_t) * (size_t)(cap + 2))) return LP_E_NOMEM;
        if (lp::launch_count(h->d_buf, nbytes, d_chunk, d_nlmask, h->line_off.as<uint64_t>(), cap, d_meta, s) != 0)
            return LP_E_DEVICE;
    }
    if (!h->line_off.ensure(sizeof(uint64_t) * (size_t)(cap + 2))) return LP_E_NOMEM;
    if (sync_count && !device) {  // the scan ran without the line index buffer: its ends now
        unsigned long long n = 0;
        hipMemcpy(&n, &d_meta->n_lines, sizeof n, hipMemcpyDeviceToHost);
        uint64_t ends[2] = {0, nbytes + 1};
        hipMemcpy(h->line_off.as<uint64_t>(), &ends[0], 8, hipMemcpyHostToDevice);
        uint8_t last = '\n';
        if (nbytes) hipMemcpy(&last, h->d_buf + nbytes - 1, 1, hipMemcpyDeviceToHost);
        if (nbytes && last != '\n' && last != '\r') hipMemcpy(h->line_off.as<uint64_t>() + n, &ends[1], 8, hipMemcpyHostToDevice);
    }
    h->cap_lines = cap;
    if (!device && lp::launch_offsets(d_nlmask, nbytes, d_chunk, h->line_off.as<uint64_t>(), cap, s) != 0)
        return LP_E_DEVICE;
    hipEventRecord(h->ev[1], s);
    if (!alloc_columns(h, cap)) return LP_E_NOMEM;
    // arena: ARENA_SHARDS shards of shard_cap bytes; the reservation is a
    // minimum (a re-run after an overflow needs the grown estimate)
    const double per = h->arena_per_line > 0 ? h->arena_per_line * 1.25 : 64.0;
    uint64_t acap = std::max<uint64_t>(h->reserve_arena, (uint64_t)(per * (double)cap) + (1u << 20));
    if (h->arena_first && h->retries == 0) acap = h->arena_first;
    if (!device || !P.has_phase2()) acap = 4096 * LP_ARENA_SHARDS;
    h->shard_cap = (acap / LP_ARENA_SHARDS + 255) & ~255ull;
    if (!h->arena.ensure(h->shard_cap * LP_ARENA_SHARDS)) return LP_E_NOMEM;
    lp::Columns& C = h->C;
    C.line_off = h->line_off.as<uint64_t>();
    C.arena = h->arena.as<uint8_t>();
    C.shard_cap = h->shard_cap;
    C.meta = d_meta;
    C.cap_lines = cap;
    const int64_t waves = lp::parse_waves(cap);
    if (!h->waves.ensure(4 * lp::WC_WORDS * (size_t)(waves + 1))) return LP_E_NOMEM;
    if (!h->ovf.ensure(4 * (size_t)(waves + 1) + 4 * (size_t)(cap + 1))) return LP_E_NOMEM;
    C.wave_counts = h->waves.as<uint32_t>();
    C.uri_ovf_list = h->ovf.as<uint32_t>();
    C.uri_fix_list = h->ovf.as<uint32_t>() + (waves + 1);  // one entry per line
    if (device) {
        if (P.n_fmt > 1) {  // sticky multi-format routing scratch
            if (!h->route.ensure(8 * (size_t)(lp::fmt_chunks(cap) + 1))) return LP_E_NOMEM;
            C.fmt_chunk = h->route.as<uint64_t>();
            C.fmt_init = h->fmt_state;
        }
        if (!h->args.ensure(sizeof(lp::DeviceArgs))) return LP_E_NOMEM;
        lp::ParseLaunch pl{h->d_buf, nbytes, cap, (uint64_t)(h->mean_line > 0 ? h->mean_line + 0.5 : 0),
                           P.n_elems, P.max_stack, h->force_direct, P.has_phase2(), false, P.n_uri, P.n_query,
                           h->ev[4]};
        for (int u = 0; u < P.n_uri; ++u) pl.derived = pl.derived || P.uri[u].src_q >= 0;
        // ... and the value stages that have a guard there (a parameter's occurrences, a SCREENRESOLUTION's parts)
        for (int k = 0; k < P.n_val; ++k) pl.derived = pl.derived || P.val[k].src_q >= 0 || P.val[k].kind == lp::VK_SCREEN;
        if (!pl.mean_line && cap > 0) pl.mean_line = (nbytes + cap - 1) / (uint64_t)cap;
        pl.chunk_lines = h->chunk_lines;
        pl.chunk_wait = h->chunk_wait;
        pl.multi = P.n_fmt > 1;
        pl.lit_aware = false;
        for (int i = 0; i < P.n_elems; ++i) {
            const lp::ElemV e = lp::load_elem(P.elems + i);
            if (e.nlit && !e.last && ((e.kind == lp::EK_NOSPACE && !e.det) || e.kind == lp::EK_NOSPACE3))
                pl.lit_aware = true;
        }
        for (int k = 0; k < P.n_val; ++k) pl.geoip = pl.geoip || P.val[k].kind == lp::VK_GEOIP;
        pl.geo_event[0] = h->ev[5];
        pl.geo_event[1] = h->ev[6];
        pl.simple = simple_program(P);
        pl.shape = h->fixed_shape && !pl.lit_aware ? fixed_shape_program(P, h->force_direct) : lp::FS_NONE;
        h->last_launch = pl;
        // look-back words (zeroed), per-chunk counts, the queued line list
        const lp::ChunkPlan cp = lp::chunk_plan(pl);
        const size_t sb = align256(8 * (size_t)(cp.n_chunks + 1)), cb = align256(4 * lp::WC_WORDS * (size_t)(cp.n_chunks + 1));
        const size_t ob = align256(4 * (size_t)(cap + 1));
        if (!h->cstate.ensure(sb + cb + ob + 4 * (size_t)(cp.n_chunks + 1))) return LP_E_NOMEM;
        C.chunk_state = h->cstate.as<uint64_t>();
        C.chunk_counts = h->cstate.as<uint32_t>(sb);
        C.ovf_lines = h->cstate.as<uint32_t>(sb + cb);
        C.deferred_chunks = h->cstate.as<uint32_t>(sb + cb + ob);
        if (hipMemsetAsync(C.chunk_state, 0, sb, s) != hipSuccess) return LP_E_DEVICE;
        h->host_args.prog = P;
        h->host_args.cols = C;
        if (hipMemcpyAsync(h->args.p, &h->host_args, sizeof(lp::DeviceArgs), hipMemcpyHostToDevice, s) != hipSuccess)
            return LP_E_DEVICE;
        hipEventRecord(h->ev[2], s);
        const lp::DeviceArgs* d_args = h->args.as<lp::DeviceArgs>();
        if (lp::launch_parse(pl, d_args, C, s) != 0) return LP_E_DEVICE;
    } else {
        // the requested paths need a dissector that is not on the device:
        // every line goes back to the reference (FALLBACK)
        hipEventRecord(h->ev[2], s);
        if (cap) hipMemsetAsync(C.status, LP_LINE_FALLBACK, (size_t)cap, s);
        hipEventRecord(h->ev[4], s);
    }
    hipEventRecord(h->ev[3], s);
    return LP_OK;
}

// Wait for the batch, read its bookkeeping; when its line count or arena
// need outgrew the buffers, re-run it with exact sizes.
int finish(lp_handle* h) {
    int cap_reruns = 0;    // re-runs for a short line capacity: always (the re-run has the exact count)
    int arena_reruns = 0;  // ... for a short arena: at most LP_OPT_MAX_RETRIES
    for (;;) {
        if (hipStreamSynchronize(h->stream) != hipSuccess) return LP_E_DEVICE;
        lp::Meta m;
        if (hipMemcpy(&m, h->meta.p, sizeof m, hipMemcpyDeviceToHost) != hipSuccess) return LP_E_DEVICE;
        if (m.err) {
            // a kernel's self-check of its own bookkeeping failed (parse.hip check_fail)
            fprintf(stderr,
                    "logparser_amd: internal check failed %llu time(s); first: kind %llu values %llu %llu %llu %llu "
                    "(batch %llu bytes, %llu lines)\n",
                    m.err, m.err_info[0], m.err_info[1], m.err_info[2], m.err_info[3], m.err_info[4],
                    (unsigned long long)h->nbytes, m.n_lines);
            if (m.err_info[0] == 2) {
                const lp::ChunkPlan cp = lp::chunk_plan(h->last_launch);
                fprintf(stderr,
                        "  chunk_excess received w0 %llu w1 %llu t_lo %llu t_hi %llu first %llu win %llx nbytes %llu "
                        "buf %llx (host: buf %llx cb %u win_cap %u)\n",
                        m.err_info[5], m.err_info[6], m.err_info[7], m.err_info[8], m.err_info[9], m.err_info[10],
                        m.err_info[11], m.err_info[12], (unsigned long long)(uintptr_t)h->d_buf, cp.cb, cp.win_cap);
            }
            return LP_E_DEVICE;
        }
        uint64_t top_max = 0;
        for (int s = 0; s < LP_ARENA_SHARDS; ++s) {
            h->shard_top[s] = m.shard_top[16 * s];
            top_max = std::max<uint64_t>(top_max, h->shard_top[s]);
        }
        const int64_t n = (int64_t)m.n_lines;
        // LP_OPT_MAX_RETRIES bounds the arena re-runs only: a short arena has
        // a fallback (its lines go FALLBACK), a short line capacity has none
        const bool cap_rerun = m.cap_ovf && cap_reruns < 2;
        const bool arena_rerun = !m.cap_ovf && m.arena_ovf && arena_reruns < h->max_retries;
        if (h->plan.device_ok() && (cap_rerun || arena_rerun)) {
            // exact sizes: the line count, every shard as large as the largest
            // request (shard tops count what was asked for, also past the end)
            if (cap_rerun) ++cap_reruns;
            else ++arena_reruns;
            ++h->retries;
            h->cap_lines = std::max<int64_t>(n, h->cap_lines);
            if (n > 0) h->mean_line = (double)h->nbytes / (double)n;
            // the next estimate (arena_per_line x 1.25 x capacity) covers the largest shard
            if (m.arena_ovf && n > 0)
                h->arena_per_line = std::max(h->arena_per_line, (double)(top_max + 4096) * LP_ARENA_SHARDS / (double)n);
            const int st = enqueue(h, false);
            if (st != LP_OK) return st;
            continue;
        }
        // more lines than columns: nothing was parsed.  An arena that is still
        // short after the re-runs degrades instead: the lines whose region or
        // pieces did not fit are FALLBACK (the kernels marked them), the rest
        // of the batch is delivered
        if (m.cap_ovf) return LP_E_NOMEM;
        h->arena_ovf = m.arena_ovf;
        h->n_lines = n;
        if (h->plan.device_ok()) {
            for (int k = 0; k < 4; ++k) h->counters[k] = m.counters[k];
            h->arena_written = m.counters[4];
            h->uri_src_bytes = m.counters[5];
            h->ovf_lines = m.ovf_lines;
            h->uri_ovf_waves = m.uri_ovf_waves;
            h->deferred = m.deferred;
            h->dfs_lines = m.dfs_lines;
            h->walk_lines = m.walk_lines;
            h->uri_fix_lines = (m.uri_fix_lines & 0xFFFFFFFFull) + (m.uri_fix_lines >> 32);  // the queued ones, k_uri_overflow's own
        } else {
            h->counters[0] = (uint64_t)n;
            h->counters[1] = h->counters[2] = 0;
            h->counters[3] = (uint64_t)n;
            h->arena_written = 0;
            h->uri_src_bytes = 0;
        }
        for (int s = 0; s < LP_ARENA_SHARDS; ++s) h->shard_top[s] = std::min<uint64_t>(h->shard_top[s], h->shard_cap);
        const lp::Program& P = h->plan.program();
        if (h->plan.device_ok() && P.n_fmt > 1 && n > 0) h->fmt_state = (uint32_t)m.fmt_state;
        if (n > 0) {
            h->mean_line = (double)h->nbytes / (double)n;
            h->arena_per_line = (double)top_max * LP_ARENA_SHARDS / (double)n;
        }
        float a = 0, b = 0, c = 0, d = 0, e = 0;
        hipEventElapsedTime(&a, h->ev[0], h->ev[3]);
        hipEventElapsedTime(&b, h->ev[0], h->ev[1]);
        hipEventElapsedTime(&c, h->ev[2], h->ev[3]);
        hipEventElapsedTime(&d, h->ev[2], h->ev[4]);
        hipEventElapsedTime(&e, h->ev[4], h->ev[3]);
        h->ms[0] = a; h->ms[1] = b; h->ms[2] = c; h->ms[3] = d; h->ms[4] = e;
        h->geo_ms = 0;
        if (h->plan.device_ok() && h->last_launch.geoip && lp::parse_waves(h->cap_lines) > 0)
            hipEventElapsedTime(&h->geo_ms, h->ev[5], h->ev[6]);
        return LP_OK;
    }
}

int ensure_synced(lp_handle* h) {
    if (h->pending) {
        const int st = lp_sync(h);
        if (st != LP_OK) return st;
    }
    return h->valid ? LP_OK : LP_E_STATE;
}

// Bytes of a host copy (line index, columns, arena shards, input) and its
// layout; fills r when dst is non-null.
int64_t copy_result(lp_handle* h, uint8_t* dst, uint64_t cap, bool with_input, lp_result* r) {
    const int64_t n = h->n_lines;
    uint64_t cols_bytes = 0;
    // the column table travels in the copy: the result never points into the
    // handle (a later copy or batch must not invalidate an earlier copy)
    const std::vector<lp_column> cols = layout(h->specs, n, &cols_bytes);
    const uint64_t tab_bytes = sizeof(lp_column) * cols.size();
    uint64_t arena_bytes = 0;
    uint64_t shard_off[LP_ARENA_SHARDS];
    for (int s = 0; s < LP_ARENA_SHARDS; ++s) {
        shard_off[s] = arena_bytes;
        arena_bytes += (h->shard_top[s] + 15) & ~15ull;
    }
    const uint64_t o_tab = 0, o_lines = align256(tab_bytes), o_cols = o_lines + align256(8 * (uint64_t)(n + 1));
    const uint64_t o_arena = o_cols + cols_bytes;
    const uint64_t o_input = align256(o_arena + arena_bytes);
    const uint64_t total = with_input ? o_input + h->nbytes + 64 : o_input;
    if (!dst) return -(int64_t)total;
    if (cap < total) return -(int64_t)total;
    auto cp = [&](uint64_t off, const void* src, uint64_t bytes) {
        return bytes == 0 || hipMemcpy(dst + off, src, bytes, hipMemcpyDeviceToHost) == hipSuccess;
    };
    if (tab_bytes) memcpy(dst + o_tab, cols.data(), tab_bytes);
    bool ok = cp(o_lines, h->line_off.p, 8 * (uint64_t)(n + 1));
    for (size_t k = 0; k < h->specs.size() && ok; ++k)
        ok = cp(o_cols + cols[k].offset, *h->specs[k].field, (uint64_t)h->specs[k].esz * (uint64_t)n);
    for (int s = 0; s < LP_ARENA_SHARDS && ok; ++s)
        ok = cp(o_arena + shard_off[s], h->arena.as<uint8_t>((size_t)s * h->shard_cap), h->shard_top[s]);
    if (with_input && ok) {
        ok = cp(o_input, h->d_buf, h->nbytes);
        memset(dst + o_input + h->nbytes, '\n', 64);
    }
    if (!ok) return LP_E_DEVICE;
    lp_result& R = *r;
    R = lp_result{};
    R.n_lines = n;
    R.first_line = h->first_line;
    R.input_bytes = h->nbytes;
    R.input = with_input ? dst + o_input : nullptr;
    R.line_off = reinterpret_cast<const uint64_t*>(dst + o_lines);
    R.columns = dst + o_cols;
    R.columns_bytes = cols_bytes;
    R.arena = dst + o_arena;
    R.arena_bytes = arena_bytes;
    R.shard_cap = h->shard_cap;
    for (int s = 0; s < LP_ARENA_SHARDS; ++s) R.shard_off[s] = shard_off[s];
    R.n_columns = (int32_t)cols.size();
    R.column = reinterpret_cast<const lp_column*>(dst + o_tab);
    R.on_host = 1;
    return (int64_t)total;
}

bool fetch_host(lp_handle* h) {
    if (h->host_valid) return true;
    if (ensure_synced(h) != LP_OK) return false;
    const int64_t need = -copy_result(h, nullptr, 0, true, nullptr);
    h->hostbuf.resize((size_t)need);
    if (copy_result(h, h->hostbuf.data(), (uint64_t)need, true, &h->host_res) < 0) return false;
    make_view(h, h->host_res, h->view);
    h->host_valid = true;
    return true;
}

}  // namespace

extern "C" {

lp_handle* lp_compile(const char* logformats, const char* const* paths, int n_paths, int device, int* status,
                      char* err, size_t errlen) {
    return lp_compile_remapped(logformats, paths, n_paths, nullptr, 0, device, status, err, errlen);
}

lp_handle* lp_compile_remapped(const char* logformats, const char* const* paths, int n_paths, const lp_remap* remaps,
                               int n_remaps, int device, int* status, char* err, size_t errlen) {
    return lp_compile_dissectors(logformats, paths, n_paths, remaps, n_remaps, nullptr, 0, device, status, err, errlen);
}

lp_handle* lp_compile_dissectors(const char* logformats, const char* const* paths, int n_paths, const lp_remap* remaps,
                                 int n_remaps, const lp_dissector* dissectors, int n_dissectors, int device, int* status,
                                 char* err, size_t errlen) {
    if (status) *status = LP_E_INVALID;
    if (!logformats || (n_paths > 0 && !paths) || (n_remaps > 0 && !remaps) || (n_dissectors > 0 && !dissectors)) {
        set_err(err, errlen, "null argument");
        return nullptr;
    }
    std::vector<lp::AddDissector> dz;
    for (int i = 0; i < n_dissectors; ++i) {
        if (!dissectors[i].name) { set_err(err, errlen, "null dissector name"); return nullptr; }
        dz.push_back(lp::AddDissector{dissectors[i].name, dissectors[i].settings ? dissectors[i].settings : ""});
    }
    std::vector<lp::Remap> rm;
    for (int i = 0; i < n_remaps; ++i) {
        if (!remaps[i].input || !remaps[i].type) { set_err(err, errlen, "null remapping"); return nullptr; }
        rm.push_back(lp::Remap{remaps[i].input, remaps[i].type, (int)remaps[i].casts});
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
        if (status) *status = LP_E_DEVICE;
        set_err(err, errlen, "logparser_amd: no HIP device available (the engine runs only on the GPU)");
        return nullptr;
    }
    if (device < 0 || device >= ndev) { if (status) *status = LP_E_DEVICE; set_err(err, errlen, "bad device ordinal"); return nullptr; }
    auto h = std::make_unique<lp_handle>();
    h->device = device;
    std::vector<std::string> f;
    for (int i = 0; i < n_paths; ++i) f.emplace_back(paths[i]);
    std::string e;
    int st = h->plan.build(logformats, f, e, rm, dz);
    if (st != LP_OK && st != LP_E_UNSUPPORTED) {
        if (status) *status = st;
        set_err(err, errlen, e);
        return nullptr;
    }
    if (st == LP_E_UNSUPPORTED) set_err(err, errlen, h->plan.unsupported_reason());
    h->compile_status = st;
    build_specs(h.get());
    if (hipSetDevice(device) != hipSuccess) { if (status) *status = LP_E_DEVICE; return nullptr; }
    for (auto& ev : h->ev) hipEventCreate(&ev);
    for (auto& ev : h->tev) hipEventCreate(&ev);
    h->have_events = true;
    if (!h->meta.ensure(sizeof(lp::Meta))) { if (status) *status = LP_E_NOMEM; return nullptr; }
    if (st == LP_OK && !upload_geo(h.get())) {
        lp_handle* raw = h.release();
        lp_free(raw);
        if (status) *status = LP_E_NOMEM;
        set_err(err, errlen, "no device memory for the GeoIP images");
        return nullptr;
    }
    if (status) *status = st;
    return h.release();
}

void lp_free(lp_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->pending) hipStreamSynchronize(h->stream);
    for (auto* b : {&h->input, &h->chunk, &h->line_off, &h->cols, &h->arena, &h->meta, &h->waves, &h->args, &h->route,
                    &h->ovf, &h->hist, &h->cstate, &h->targs, &h->tscratch, &h->gacc})
        b->release();
    for (auto& b : h->geo_tree) b.release();
    for (auto& b : h->geo_fields) b.release();
    for (auto& b : h->geo_pool) b.release();
    if (h->have_events) {
        for (auto& ev : h->ev) hipEventDestroy(ev);
        for (auto& ev : h->tev) hipEventDestroy(ev);
    }
    delete h;
}

int64_t lp_possible_paths(const char* logformats, int max_depth, char* out, size_t cap) {
    return lp_possible_paths_remapped(logformats, max_depth, nullptr, 0, out, cap);
}

int64_t lp_possible_paths_remapped(const char* logformats, int max_depth, const lp_remap* remaps, int n_remaps,
                                   char* out, size_t cap) {
    return lp_possible_paths_dissectors(logformats, max_depth, remaps, n_remaps, nullptr, 0, out, cap);
}

int64_t lp_possible_paths_dissectors(const char* logformats, int max_depth, const lp_remap* remaps, int n_remaps,
                                     const lp_dissector* dissectors, int n_dissectors, char* out, size_t cap) {
    if ((n_remaps > 0 && !remaps) || (n_dissectors > 0 && !dissectors)) return LP_E_INVALID;
    std::vector<lp::AddDissector> dz;
    for (int i = 0; i < n_dissectors; ++i) {
        if (!dissectors[i].name) return LP_E_INVALID;
        dz.push_back(lp::AddDissector{dissectors[i].name, dissectors[i].settings ? dissectors[i].settings : ""});
    }
    std::vector<lp::Remap> rm;
    for (int i = 0; i < n_remaps; ++i) {
        if (!remaps[i].input || !remaps[i].type) return LP_E_INVALID;
        rm.push_back(lp::Remap{remaps[i].input, remaps[i].type, (int)remaps[i].casts});
    }
    std::vector<std::string> paths;
    std::string err;
    if (lp::Plan::possible_paths(logformats ? logformats : "", max_depth, paths, err, rm, dz) != LP_OK) return LP_E_INVALID;
    std::string s;
    for (auto& p : paths) s += p + "\n";
    if (!out || s.size() + 1 > cap) return -(int64_t)(s.size() + 1);
    memcpy(out, s.c_str(), s.size() + 1);
    return (int64_t)s.size();
}

int lp_set_option(lp_handle* h, int option, int64_t value) {
    if (!h) return LP_E_INVALID;
    switch (option) {
    case LP_OPT_FORCE_DIRECT: h->force_direct = value != 0; return LP_OK;
    case LP_OPT_CHUNK_LINES:
        if (value < 0 || value > 64) return LP_E_INVALID;
        h->chunk_lines = (uint32_t)value;
        return LP_OK;
    case LP_OPT_ONE_PASS: return value == 1 ? LP_OK : LP_E_INVALID;  // (the only mode; 1 changes nothing)
    case LP_OPT_FIXED_SHAPE:
        h->fixed_shape = value != 0;
        return LP_OK;
    case LP_OPT_CHUNK_WAIT:
        h->chunk_wait = value == -2 ? -2 : value < 0 ? -1 : (int32_t)std::min<int64_t>(value, 1 << 30);
        return LP_OK;
    case LP_OPT_MAX_RETRIES:
        if (value < 0 || value > 16) return LP_E_INVALID;
        h->max_retries = (int)value;
        return LP_OK;
    case LP_OPT_ARENA_BYTES:
        if (value < 0) return LP_E_INVALID;
        h->arena_first = (uint64_t)value;
        return LP_OK;
    case LP_OPT_DICT_HASH_BITS:
        if (value < 0 || value > 32) return LP_E_INVALID;
        h->dict_hash_bits = (int)value;
        return LP_OK;
    case LP_OPT_GROUP_LDS_WORDS:
        if (value < -1 || value > lp::GROUP_LDS_WORDS_MAX) return LP_E_INVALID;
        h->group_lds_words = (int)value;
        return LP_OK;
    case LP_OPT_GROUP_PEEL:
        if (value < -1 || value > lp::GROUP_PEEL_MAX) return LP_E_INVALID;
        h->group_peel = (int)value;
        return LP_OK;
    default: return LP_E_INVALID;
    }
}

int lp_reserve(lp_handle* h, int64_t max_lines, uint64_t arena_bytes) {
    if (!h || max_lines < 0) return LP_E_INVALID;
    h->reserve_lines = max_lines;
    h->reserve_arena = arena_bytes;
    if (max_lines > h->cap_lines) h->cap_lines = max_lines;
    return LP_OK;
}

int lp_parse_batch(lp_handle* h, const uint8_t* buf, uint64_t nbytes, int buf_flags, void* stream) {
    if (!h) return LP_E_INVALID;
    if (h->pending) lp_sync(h);  // the previous batch's line count continues the numbering
    return lp_parse_batch_at(h, buf, nbytes, h->next_line, buf_flags, stream);
}

int lp_parse_batch_at(lp_handle* h, const uint8_t* buf, uint64_t nbytes, int64_t first_line_no, int buf_flags,
                      void* stream) {
    if (!h || (!buf && nbytes) || first_line_no < 0) return LP_E_INVALID;
    if (hipSetDevice(h->device) != hipSuccess) return LP_E_DEVICE;
    if (h->pending) lp_sync(h);
    // the handle holds no valid batch until this one has been enqueued
    h->valid = false;
    h->host_valid = false;
    h->n_lines = 0;
    h->retries = 0;
    h->arena_ovf = 0;
    h->first_line = h->next_line = first_line_no;
    hipStream_t s = (hipStream_t)stream;
    h->stream = s;
    h->nbytes = nbytes;
    if (buf_flags == LP_BUF_HOST) {
        if (!h->input.ensure(nbytes + 16)) return LP_E_NOMEM;
        if (nbytes && hipMemcpyAsync(h->input.p, buf, nbytes, hipMemcpyHostToDevice, s) != hipSuccess) return LP_E_DEVICE;
        h->d_buf = h->input.as<uint8_t>();
    } else if (((uintptr_t)buf & 15u) != 0) {
        // the index and staging passes stream 16-byte aligned loads; a batch
        // that starts mid-word (a line-aligned slice of a larger buffer) is
        // first copied to the handle's aligned buffer (measured: misaligned
        // streaming ran the index 4.5x and the parse kernel 2.2x slower)
        if (!h->input.ensure(nbytes + 16)) return LP_E_NOMEM;
        if (nbytes && hipMemcpyAsync(h->input.p, buf, nbytes, hipMemcpyDeviceToDevice, s) != hipSuccess) return LP_E_DEVICE;
        h->d_buf = h->input.as<uint8_t>();
    } else {
        h->d_buf = buf;
    }
    // capacity from the reservation or the previous batch's line length; a
    // handle without either counts its lines first (one synchronisation)
    bool sync_count = false;
    if (h->reserve_lines > 0) {
        h->cap_lines = std::max<int64_t>(h->cap_lines, h->reserve_lines);
    } else if (h->mean_line > 0) {
        const int64_t est = headroom((int64_t)((double)nbytes / h->mean_line));
        h->cap_lines = std::max<int64_t>(h->cap_lines, est);
    } else {
        sync_count = true;
    }
    const int st = enqueue(h, sync_count);
    if (st != LP_OK) return st;
    h->pending = true;
    h->valid = true;
    return LP_OK;
}

int lp_sync(lp_handle* h) {
    if (!h) return LP_E_INVALID;
    if (!h->pending) return h->valid ? LP_OK : LP_E_STATE;
    hipSetDevice(h->device);
    h->pending = false;
    const int st = finish(h);
    if (st != LP_OK) {
        h->valid = false;
        h->n_lines = 0;
    } else {
        h->next_line = h->first_line + h->n_lines;
    }
    return st;
}

int64_t lp_num_lines(lp_handle* h) {
    if (!h) return LP_E_INVALID;
    const int st = ensure_synced(h);
    return st == LP_OK ? h->n_lines : st;
}

int lp_line_status(lp_handle* h, int64_t first, int64_t count, uint8_t* out) {
    if (!h) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    if (first < 0 || count < 0 || first + count > h->n_lines || (count && !out)) return LP_E_INVALID;
    if (!count) return LP_OK;
    if (h->host_valid) {  // served from the host copy
        memcpy(out, h->view.status + first, (size_t)count);
        return LP_OK;
    }
    if (hipMemcpy(out, h->C.status + first, (size_t)count, hipMemcpyDeviceToHost) != hipSuccess) return LP_E_DEVICE;
    return LP_OK;
}

int64_t lp_line_offset(lp_handle* h, int64_t i) {
    if (!h) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    if (i < 0 || i > h->n_lines) return LP_E_INVALID;
    if (h->host_valid) return (int64_t)h->view.line_off[i];
    uint64_t v = 0;
    if (hipMemcpy(&v, h->line_off.as<uint64_t>() + i, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return LP_E_DEVICE;
    return (int64_t)v;
}

int64_t lp_line_record_json(lp_handle* h, int64_t i, char* out, size_t cap) {
    if (!h) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    if (i < 0 || i >= h->n_lines) return LP_E_INVALID;
    if (!fetch_host(h)) return LP_E_DEVICE;
    if (h->view.status[i] != LP_LINE_OK) return LP_E_STATE;
    std::string js = h->plan.record_json(h->view, i);
    if (!out || js.size() + 1 > cap) return -100 - (int64_t)(js.size() + 1);
    memcpy(out, js.c_str(), js.size() + 1);
    return (int64_t)js.size();
}

int lp_counters(lp_handle* h, uint64_t* out, int n) {
    if (!h || !out) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    const uint64_t v[13] = {h->counters[0], h->counters[1], h->counters[2], h->counters[3], h->ovf_lines,
                            (uint64_t)h->retries, h->arena_ovf, h->uri_ovf_waves, h->deferred, h->dfs_lines,
                            h->uri_fix_lines, (uint64_t)h->last_launch.shape, h->walk_lines};
    for (int k = 0; k < n && k < 13; ++k) out[k] = v[k];
    return n < 13 ? n : 13;
}

int lp_histograms(lp_handle* h, uint64_t* out, int out_on_device) {
    if (!h || !out) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    if (!h->valid) return LP_E_INVALID;
    static_assert(lp::HIST_WORDS == LP_HIST_WORDS, "histogram layout");
    if (!h->plan.device_ok()) {  // every line FALLBACK
        std::vector<uint64_t> v(LP_HIST_WORDS, 0);
        v[LP_HIST_LINES] = h->counters[0];
        v[LP_HIST_FALLBACK] = h->counters[3];
        if (!out_on_device) memcpy(out, v.data(), 8 * v.size());
        else if (hipMemcpy(out, v.data(), 8 * v.size(), hipMemcpyHostToDevice) != hipSuccess) return LP_E_DEVICE;
        return LP_OK;
    }
    uint64_t* d = out;
    if (!out_on_device) {
        if (!h->hist.ensure(8 * (size_t)LP_HIST_WORDS)) return LP_E_NOMEM;
        d = h->hist.as<uint64_t>();
    }
    if (lp::launch_histograms(h->args.as<lp::DeviceArgs>(), h->d_buf, h->n_lines, d, h->stream) != 0) return LP_E_DEVICE;
    if (!out_on_device && hipMemcpyAsync(out, d, 8 * (size_t)LP_HIST_WORDS, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
        return LP_E_DEVICE;
    return hipStreamSynchronize(h->stream) == hipSuccess ? LP_OK : LP_E_DEVICE;
}

int lp_last_timing(lp_handle* h, float* out, int n) {
    if (!h || !out) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    for (int k = 0; k < n && k < 5; ++k) out[k] = h->ms[k];
    for (int k = 5; k < n && k < 16; ++k) out[k] = h->tms[k - 5];
    if (n < 17) return n < 16 ? n : 16;  // (a caller of the 16 values sees what it always saw)
    out[16] = h->tms[TMS_ARROW];
    if (n < 18) return 17;
    out[17] = h->geo_ms;
    if (n < 20) return 18;  // (a caller of the 18 values sees what it always saw)
    out[18] = h->tms[TMS_WHERE];
    out[19] = h->tms[TMS_WHERE + 1];
    if (n < 23) return 20;  // (a caller of the 20 values sees what it always saw)
    for (int k = 0; k < 3; ++k) out[20 + k] = h->tms[TMS_GROUP + k];
    return 23;
}

int lp_last_bytes(lp_handle* h, uint64_t* out, int n) {
    if (!h || !out) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    uint64_t row = 8;  // line index entry
    uint64_t row_uri = 0;  // the columns the URI kernels write
    for (const auto& c : h->specs) {
        row += (uint64_t)c.esz;
        if (c.uri) row_uri += (uint64_t)c.esz;
    }
    const uint64_t n1 = (uint64_t)h->n_lines;
    const lp::Program& P = h->plan.program();
    // parse kernels: the input once, the line index, their columns;
    // URI kernels: the gathered URI bytes, per line the status, line start,
    // token flags and one source span per URI stage, their columns and arena
    const uint64_t parse_b = h->nbytes + 8 * (n1 + 1) + n1 * (row - 8 - row_uri);
    // (a redone line, uri_redo_line: the line read again from HBM, a mean
    // line's bytes, and its URI columns written again; its second region is
    // in arena_written)
    const uint64_t redo_b = h->uri_fix_lines * ((n1 ? h->nbytes / n1 : 0) + row_uri);
    const uint64_t uri_b = P.has_phase2() ? h->uri_src_bytes + n1 * (1 + 8 + 4 + 4 * (uint64_t)P.n_uri) + n1 * row_uri +
                                         h->arena_written + redo_b : 0;
    uint64_t v[4] = {h->nbytes, n1 * row + h->arena_written, parse_b, uri_b};
    for (int k = 0; k < n && k < 4; ++k) out[k] = v[k];
    return n < 4 ? n : 4;
}

int lp_casts(lp_handle* h, const char* target) {
    if (!h || !target) return LP_E_INVALID;
    const int c = h->plan.casts(target);
    return c < 0 ? LP_E_MISSING : c;
}

int64_t lp_describe(lp_handle* h, char* out, size_t cap) {
    if (!h) return LP_E_INVALID;
    std::string d = h->plan.describe();
    if (!out || d.size() + 1 > cap) return -(int64_t)(d.size() + 1);
    memcpy(out, d.c_str(), d.size() + 1);
    return (int64_t)d.size();
}

int lp_result_view(lp_handle* h, lp_result* out) {
    if (!h || !out) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    lp_result& R = *out;
    R = lp_result{};
    R.n_lines = h->n_lines;
    R.first_line = h->first_line;
    R.input_bytes = h->nbytes;
    R.input = h->d_buf;
    R.line_off = h->line_off.as<uint64_t>();
    R.columns = h->cols.as<uint8_t>();
    R.columns_bytes = h->cols.cap;
    R.arena = h->arena.as<uint8_t>();
    R.arena_bytes = h->shard_cap * LP_ARENA_SHARDS;
    R.shard_cap = h->shard_cap;
    for (int s = 0; s < LP_ARENA_SHARDS; ++s) R.shard_off[s] = (uint64_t)s * h->shard_cap;
    R.n_columns = (int32_t)h->dev_cols.size();
    R.column = h->dev_cols.data();
    R.on_host = 0;
    return LP_OK;
}

int64_t lp_result_copy(lp_handle* h, void* host, uint64_t cap, int with_input, lp_result* out) {
    if (!h || (host && !out)) return LP_E_INVALID;
    const int st = ensure_synced(h);
    if (st != LP_OK) return st;
    return copy_result(h, (uint8_t*)host, host ? cap : 0, with_input != 0, out);
}

int64_t lp_result_record_json(lp_handle* h, const lp_result* r, int64_t i, char* out, size_t cap) {
    if (!h || !r || !r->on_host || !r->input) return LP_E_INVALID;
    if (i < 0 || i >= r->n_lines) return LP_E_INVALID;
    lp::ResultView V;
    make_view(h, *r, V);
    if (!V.status || V.status[i] != LP_LINE_OK) return LP_E_STATE;
    std::string js = h->plan.record_json(V, i);
    if (!out || js.size() + 1 > cap) return -100 - (int64_t)(js.size() + 1);
    memcpy(out, js.c_str(), js.size() + 1);
    return (int64_t)js.size();
}

// ---- typed columns of a batch (the output side: ParsedRecord / the Hive SerDe)
namespace {
// Long.parseLong: optional sign, decimal digits only, in range
bool java_parse_long(const uint8_t* p, uint32_t n, int64_t& out) {
    uint32_t k = 0;
    bool neg = false;
    if (n && (p[0] == '-' || p[0] == '+')) { neg = p[0] == '-'; k = 1; }
    if (k == n) return false;
    unsigned __int128 v = 0;
    for (; k < n; ++k) {
        if (p[k] < '0' || p[k] > '9') return false;
        v = v * 10 + (p[k] - '0');
        if (v > ((unsigned __int128)1 << 63)) return false;
    }
    if (!neg && v == ((unsigned __int128)1 << 63)) return false;
    out = neg ? (int64_t)(0 - (uint64_t)v) : (int64_t)v;
    return true;
}
// Double.parseDouble (FloatingDecimal.readJavaFormatString): chars <= ' '
// trimmed; [+-] then NaN | Infinity | decimal digits with an optional '.',
// exponent and f/F/d/D suffix | a hex float with a binary exponent
bool java_parse_double(const uint8_t* p, uint32_t n, double& out) {
    uint32_t a = 0, b = n;
    while (a < b && p[a] <= ' ') ++a;
    while (b > a && p[b - 1] <= ' ') --b;
    std::string t((const char*)p + a, b - a);
    static const std::regex dec("[+-]?(NaN|Infinity|(([0-9]+\\.?[0-9]*|\\.[0-9]+)([eE][+-]?[0-9]+)?)[fFdD]?)");
    static const std::regex hex("[+-]?0[xX]([0-9a-fA-F]+\\.?[0-9a-fA-F]*|\\.[0-9a-fA-F]+)[pP][+-]?[0-9]+[fFdD]?");
    const bool d = std::regex_match(t, dec), x = !d && std::regex_match(t, hex);
    if (!d && !x) return false;
    const bool neg = !t.empty() && t[0] == '-';
    if (t.find("NaN") != std::string::npos) { out = std::nan(""); return true; }
    if (t.find("Infinity") != std::string::npos) { out = neg ? -HUGE_VAL : HUGE_VAL; return true; }
    if (!t.empty() && strchr("fFdD", t.back())) t.pop_back();
    out = strtod(t.c_str(), nullptr);
    return true;
}
struct TableCtx {
    const std::unordered_map<std::string, std::vector<int>>* by_path;
    lp_table_col* cols;
    int64_t row;           // row in the output
    std::vector<std::string>* sbuf;  // per column: this chunk's STRING bytes
    std::vector<std::vector<std::pair<uint64_t, uint32_t>>>* sref;  // per column: (offset, len) per chunk row
    int64_t row0;          // first output row of the chunk
};
void table_value(void* vctx, const std::string& target, const lp::MVal& v) {
    TableCtx& t = *(TableCtx*)vctx;
    auto it = t.by_path->find(target);
    if (it == t.by_path->end()) return;
    for (int c : it->second) {
        lp_table_col& C = t.cols[c];
        // ParsedRecord.set(name, value) (ParsedRecord.java:154-170): a null is
        // ignored, the last value wins (Value.getString / getLong / getDouble)
        if (v.null) continue;
        if (C.kind == LP_CAST_STRING) {
            std::string& buf = (*t.sbuf)[c];
            const uint64_t off = buf.size();  // a chunk's bytes of one column may pass 4 GiB
            if (v.is_long) buf += std::to_string(v.l);
            else buf.append((const char*)v.p, v.len);
            (*t.sref)[c][t.row - t.row0] = {off, (uint32_t)(buf.size() - off)};
            C.valid[t.row] = 1;
        } else if (C.kind == LP_CAST_LONG) {
            int64_t x;
            if (v.is_long) x = v.l;
            else if (!java_parse_long(v.p, v.len, x)) continue;
            C.i64[t.row] = x;
            C.valid[t.row] = 1;
        } else {
            double x;
            if (v.is_long) x = (double)v.l;
            else if (!java_parse_double(v.p, v.len, x)) continue;
            C.f64[t.row] = x;
            C.valid[t.row] = 1;
        }
    }
}
}  // namespace

// Is p memory of the handle's device (what a device view's row list must be:
// the kernels dereference it)?
static bool device_memory(lp_handle* h, const void* p) {
    hipPointerAttribute_t a{};
    hipSetDevice(h->device);
    if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (an unregistered host pointer: not a sticky error)
        return false;
    }
    return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) && a.device == h->device;
}

// ---- the checks and the plumbing the table families share.  Every family runs
// them in this order: null arguments and the columns' own arrays; each path
// (check_path); on a device view view_current, then check_rows and what only
// the device refuses (LP_E_UNSUPPORTED); on a host copy the input, then check_rows.

// A device view is only good for the batch the handle holds now
static bool view_current(lp_handle* h, const lp_result* r) {
    return !(!h->valid || r->n_lines != h->n_lines || r->first_line != h->first_line || r->input != h->d_buf ||
             r->line_off != h->line_off.as<uint64_t>());
}

// Does the plan deliver path as a column of kind (LP_CAST_*)?  A pseudo-column
// has no dissector and no casts entry: its kind is fixed.  Otherwise the casts
// of the requested path (or of its wildcard request) must allow the kind: else
// the reference's store finds no setter.  pseudo: the path's TC_* kind, 0 for none.
static int check_path(lp_handle* h, const std::string& p, int kind, int* pseudo = nullptr) {
    const int pk = lp::Plan::pseudo_kind(p);
    if (pseudo) *pseudo = pk;
    if (pk) return kind == (pk == lp::TC_LINE ? LP_CAST_STRING : LP_CAST_LONG) ? LP_OK : LP_E_INVALID;
    int casts = h->plan.casts(p);
    if (casts < 0) {
        const size_t dot = p.rfind('.');
        if (dot != std::string::npos) casts = h->plan.casts(p.substr(0, dot) + ".*");
    }
    return casts < 0 ? LP_E_MISSING : (casts & kind) ? LP_OK : LP_E_INVALID;
}

static bool check_window(int64_t first, int64_t count, const int64_t* rows, int64_t n_lines) {
    return first >= 0 && count >= 0 && (rows || first + count <= n_lines);
}

// The window, or the row list, of a call on view r.  A host list: every index
// inside the batch, before anything is written; a device list: memory of the
// handle's device (the kernels dereference it and check the indices).
static int check_rows(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows) {
    const int64_t n_lines = r->on_host ? r->n_lines : h->n_lines;
    if (!check_window(first, count, rows, n_lines)) return LP_E_INVALID;
    if (!rows) return LP_OK;
    if (!r->on_host) return count == 0 || device_memory(h, rows) ? LP_OK : LP_E_INVALID;
    for (int64_t k = 0; k < count; ++k)
        if (rows[k] < 0 || rows[k] >= n_lines) return LP_E_INVALID;
    return LP_OK;
}

// The *_rows entry points' list: null only when it is empty (then the window [0, 0))
static bool rows_arg(const int64_t*& rows, int64_t n_rows) {
    if (n_rows < 0 || (n_rows > 0 && !rows)) return false;
    if (n_rows == 0) rows = nullptr;
    return true;
}

// The table kernels' arguments of rows [first, first + count) / the row list
static std::unique_ptr<lp::TableArgs> table_args(lp_handle* h, int64_t first, int64_t count, const int64_t* rows, int n_cols) {
    auto ta = std::make_unique<lp::TableArgs>();
    memset(ta.get(), 0, sizeof(lp::TableArgs));
    ta->first = first;
    ta->count = count;
    ta->n_cols = n_cols;
    ta->rows = rows;
    ta->n_lines = h->n_lines;
    ta->first_line = h->first_line;
    return ta;
}

// table.hip's scratch of a plain table, bound into ta: the scan's storage and
// the value words, and 256 bytes after them the row-list instances' flag word
static bool bind_table_scratch(lp_handle* h, lp::TableArgs& ta, int n_str) {
    const size_t flag_at = align256(lp::table_scratch_bytes(ta.count, n_str));
    if (!h->tscratch.ensure(flag_at + 256)) return false;
    ta.srcw = reinterpret_cast<uint64_t*>((char*)h->tscratch.p + lp::table_srcw_offset(ta.count));
    ta.bad_row = reinterpret_cast<uint32_t*>((char*)h->tscratch.p + flag_at);
    return true;
}

// lp_result_table / lp_result_table_rows on a device view: the columns built
// in HBM (table.hip).  rows (device memory, null: the lines first + k): row k
// is line rows[k].
static int table_device(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                        lp_table_col* cols, int n_cols) {
    if (ensure_synced(h) != LP_OK) return LP_E_STATE;
    if (n_cols > lp::MAX_TABLE_COLS) return LP_E_INVALID;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    auto ta = table_args(h, first, count, rows, n_cols);
    std::string names;  // (Plan::table_src keeps them within TableArgs::names)
    for (int c = 0; c < n_cols; ++c) {
        lp_table_col& C = cols[c];
        lp::TableCol& T = ta->cols[c];
        T.kind = C.kind;
        if (!h->plan.table_src(C.path, T.src, names, T.alt)) return LP_E_UNSUPPORTED;
        if (C.kind == LP_CAST_DOUBLE)  // Double.parseDouble of a string stays on the host table
            for (int f = 0; f < 2 * lp::MAX_FMT; ++f) {
                const lp::TableSrc& x = f < lp::MAX_FMT ? T.src[f] : T.alt[f - lp::MAX_FMT];
                const bool long_valued = x.kind == lp::TC_NONE || x.kind == lp::TC_NULL ||
                                         (x.kind == lp::TC_URI && x.b == lp::UP_PORT) ||
                                         (x.kind == lp::TC_TIME && x.b != lp::TF_MONTHNAME && x.b != lp::TF_DATE &&
                                          x.b != lp::TF_TIME) ||
                                         x.kind == lp::TC_SECMS || x.kind == lp::TC_LIST_MS ||
                                         (x.kind == lp::TC_GEOIP && x.c != lp::GK_STRING);  // (a DOUBLE field: its f64)
                // a SECOND_MILLIS list item: digits '.' digits, parsed on the device (decimal_to_double)
                const bool decimal = x.kind == lp::TC_LIST && h->plan.program().list[x.a].secms;
                if (!long_valued && !decimal) return LP_E_UNSUPPORTED;
            }
        T.valid = C.valid;
        T.i64 = C.i64;
        T.f64 = C.f64;
        T.chars = (uint8_t*)C.chars;
    }
    memcpy(ta->names, names.data(), names.size());
    hipSetDevice(h->device);
    hipStream_t s = h->stream;
    if (!h->targs.ensure(sizeof(lp::TableArgs))) return LP_E_NOMEM;
    int n_str = 0;
    for (int c = 0; c < n_cols; ++c) n_str += cols[c].kind == LP_CAST_STRING ? 1 : 0;
    if (!bind_table_scratch(h, *ta, n_str)) return LP_E_NOMEM;
    const bool ext = lp::table_ext(*ta) && count > 0;
    if (hipMemcpyAsync(h->targs.p, ta.get(), sizeof(lp::TableArgs), hipMemcpyHostToDevice, s) != hipSuccess) return LP_E_DEVICE;
    const lp::DeviceArgs* d_args = h->args.as<lp::DeviceArgs>();
    const lp::TableArgs* d_targs = h->targs.as<lp::TableArgs>();
    PhaseTimer T{h->tev, s};  // start, values kernel done, scans done, bytes done
    T.mark(0);
    // (an empty table launches nothing and records no event of its own)
    if (lp::launch_table_values(d_args, d_targs, *ta, h->d_buf, h->tscratch.p, h->tscratch.cap, s, T.lend(1, count > 0)) != 0)
        return LP_E_DEVICE;
    T.mark(2);
    // the STRING columns' byte counts decide whether their bytes fit
    std::vector<int64_t> tot(n_cols, 0);
    for (int c = 0; c < n_cols; ++c)
        if (cols[c].kind == LP_CAST_STRING && !read_back(s, &tot[c], cols[c].i64 + count)) return LP_E_DEVICE;
    uint32_t bad_row = 0;  // a rows[k] outside the batch (its row: valid 0)
    if (ext && !read_back(s, &bad_row, ta->bad_row)) return LP_E_DEVICE;
    if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
    if (bad_row) return LP_E_INVALID;
    bool fits = true;
    for (int c = 0; c < n_cols; ++c) {
        if (cols[c].kind != LP_CAST_STRING) continue;
        cols[c].chars_len = (uint64_t)tot[c];
        if (cols[c].chars_len > cols[c].chars_cap || (tot[c] && !cols[c].chars)) fits = false;
    }
    if (!fits) return LP_E_NOMEM;
    if (lp::launch_table_chars(d_args, d_targs, *ta, h->d_buf, s) != 0) return LP_E_DEVICE;
    T.mark(3);
    if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
    if (count == 0) return LP_OK;  // (an empty call keeps the previous call's lp_last_timing [5..7])
    for (int k = 0; k < 3; ++k) h->tms[TMS_TABLE + k] = T.elapsed(k, k + 1);
    return LP_OK;
}

// lp_result_table (rows null: row k = line first + k) and lp_result_table_rows
// (row k = line rows[k], first 0, count = n_rows)
static int table_any(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                     lp_table_col* cols, int n_cols, int threads) {
    if (!h || !r || !cols || n_cols <= 0) return LP_E_INVALID;
    std::unordered_map<std::string, std::vector<int>> by_path;  // (a host copy's) path -> its columns
    std::vector<int> pseudo(n_cols, 0);  // per column: its TC_* kind when it is a pseudo-column
    for (int c = 0; c < n_cols; ++c) {  // the same validation in both modes
        const lp_table_col& C = cols[c];
        if (!C.path || !C.valid || (C.kind == LP_CAST_STRING ? !C.i64 : C.kind == LP_CAST_LONG ? !C.i64 : !C.f64))
            return LP_E_INVALID;
        if (C.kind != LP_CAST_STRING && C.kind != LP_CAST_LONG && C.kind != LP_CAST_DOUBLE) return LP_E_INVALID;
        if (const int st = check_path(h, C.path, C.kind, &pseudo[c])) return st;
        if (r->on_host && !pseudo[c]) by_path[C.path].push_back(c);
    }
    if (!r->on_host) return view_current(h, r) ? table_device(h, r, first, count, rows, cols, n_cols) : LP_E_STATE;
    if (!r->input) return LP_E_INVALID;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    lp::ResultView V;
    make_view(h, *r, V);
    const Chunks ch(count, threads);
    std::vector<std::vector<std::string>> sbuf(ch.T, std::vector<std::string>(n_cols));
    std::vector<std::vector<std::vector<std::pair<uint64_t, uint32_t>>>> sref(ch.T);
    ch.run([&](int t, int64_t a, int64_t b) {
        sref[t].assign(n_cols, std::vector<std::pair<uint64_t, uint32_t>>((size_t)(b - a), {0ull, 0u}));
        TableCtx ctx{&by_path, cols, 0, &sbuf[t], &sref[t], a};
        for (int64_t k = a; k < b; ++k) {
            for (int c = 0; c < n_cols; ++c) cols[c].valid[k] = 0;
            const int64_t i = rows ? rows[k] : first + k;
            // the pseudo-columns, from the copied line index and status: every row has them
            for (int c = 0; c < n_cols; ++c) {
                if (!pseudo[c]) continue;
                lp_table_col& C = cols[c];
                if (pseudo[c] == lp::TC_LINE) {  // the line as the parse kernels see it (kernels_common.h crlf_len)
                    const uint64_t s0 = V.line_off[i];
                    uint64_t n = V.line_off[i + 1] - 1 - s0;
                    if (n > 0 && V.input[s0 + n - 1] == '\r') --n;
                    std::string& buf = sbuf[t][c];
                    sref[t][c][(size_t)(k - a)] = {(uint64_t)buf.size(), (uint32_t)n};
                    buf.append((const char*)V.input + s0, (size_t)n);
                } else {
                    C.i64[k] = pseudo[c] == lp::TC_OFFSET ? (int64_t)V.line_off[i]
                               : pseudo[c] == lp::TC_LINENO ? r->first_line + i
                                                            : (int64_t)(V.status ? V.status[i] : LP_LINE_FALLBACK);
                }
                C.valid[k] = 1;
            }
            if (!V.status || V.status[i] != LP_LINE_OK) continue;
            ctx.row = k;
            h->plan.rec_row(V, i, table_value, &ctx);
        }
    });
    // STRING columns (Arrow layout): row k = chars[offsets[k], offsets[k + 1]),
    // the row's last value; a row without one is empty (valid 0)
    int rc = LP_OK;
    for (int c = 0; c < n_cols; ++c) {
        lp_table_col& C = cols[c];
        if (C.kind != LP_CAST_STRING) continue;
        uint64_t need = 0;
        for (int t = 0; t < ch.T; ++t)
            for (int64_t k = ch.at[t]; k < ch.at[t + 1]; ++k)
                if (C.valid[k]) need += sref[t][c][(size_t)(k - ch.at[t])].second;
        C.chars_len = need;
        if (need > C.chars_cap || (need && !C.chars)) { rc = LP_E_NOMEM; continue; }
        uint64_t pos = 0;
        for (int t = 0; t < ch.T; ++t)
            for (int64_t k = ch.at[t]; k < ch.at[t + 1]; ++k) {
                C.i64[k] = (int64_t)pos;
                if (!C.valid[k]) continue;
                const auto& pr = sref[t][c][(size_t)(k - ch.at[t])];
                memcpy(C.chars + pos, sbuf[t][c].data() + pr.first, pr.second);
                pos += pr.second;
            }
        C.i64[count] = (int64_t)pos;
    }
    return rc;
}

int lp_result_table(lp_handle* h, const lp_result* r, int64_t first, int64_t count, lp_table_col* cols, int n_cols,
                    int threads) {
    return table_any(h, r, first, count, nullptr, cols, n_cols, threads);
}

int lp_result_table_rows(lp_handle* h, const lp_result* r, const int64_t* rows, int64_t n_rows, lp_table_col* cols,
                         int n_cols, int threads) {
    return rows_arg(rows, n_rows) ? table_any(h, r, 0, n_rows, rows, cols, n_cols, threads) : LP_E_INVALID;
}

// ---- dictionary-encoded STRING columns (Arrow dictionary<int32, utf8>)

// lp_result_table_dict / lp_result_table_dict_rows on a device view: one
// column after the other in the same scratch (dict.hip; kernels.h DictLayout).
// A column: k_table_values over the rows (validity, lengths, source words; no
// offsets), the hash insert, the representatives' ranks and the indices, then
// the dictionary's values as the STRING column of the representatives' lines
// by the table's row-list instances.
static int table_dict_device(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                             lp_table_dict_col* cols, int n_cols) {
    if (ensure_synced(h) != LP_OK) return LP_E_STATE;
    if (n_cols > lp::MAX_TABLE_COLS) return LP_E_INVALID;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    for (int c = 0; c < n_cols; ++c) {  // every array the kernels write is memory of the device
        const lp_table_dict_col& C = cols[c];
        if (!device_memory(h, C.dict_off) || (count > 0 && (!device_memory(h, C.valid) || !device_memory(h, C.index))) ||
            (C.dict_chars_cap > 0 && !device_memory(h, C.dict_chars)))
            return LP_E_INVALID;
    }
    // every column's sources before anything is written
    std::vector<std::unique_ptr<lp::TableArgs>> tas;
    for (int c = 0; c < n_cols; ++c) {
        auto ta = table_args(h, first, count, rows, 1);
        std::string names;  // (Plan::table_src keeps them within TableArgs::names)
        lp::TableCol& T = ta->cols[0];
        T.kind = LP_CAST_STRING;
        if (!h->plan.table_src(cols[c].path, T.src, names, T.alt)) return LP_E_UNSUPPORTED;
        memcpy(ta->names, names.data(), names.size());
        T.valid = cols[c].valid;
        tas.push_back(std::move(ta));
    }
    hipSetDevice(h->device);
    hipStream_t s = h->stream;
    if (!h->targs.ensure(sizeof(lp::TableArgs))) return LP_E_NOMEM;
    const lp::DictLayout L = lp::dict_layout(count);
    if (!h->tscratch.ensure(L.total)) return LP_E_NOMEM;
    void* const scratch = h->tscratch.p;
    const lp::DeviceArgs* d_args = h->args.as<lp::DeviceArgs>();
    const lp::TableArgs* d_targs = h->targs.as<lp::TableArgs>();
    float ms[4] = {0, 0, 0, 0};
    int rc = LP_OK;
    for (int c = 0; c < n_cols; ++c) {
        lp_table_dict_col& C = cols[c];
        C.dict_len = 0;
        C.dict_chars_len = 0;
        if (count == 0) {  // an empty dictionary: its one offset
            if (hipMemsetAsync(C.dict_off, 0, 8, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
            continue;
        }
        lp::TableArgs& ta = *tas[c];
        lp::DictArgs da{};
        da.count = count;
        da.hash_bits = h->dict_hash_bits;
        da.valid = C.valid;
        da.index = C.index;
        lp::dict_bind(da, ta, L, scratch);
        const bool ext = lp::table_ext(ta);
        if (hipMemcpyAsync(h->targs.p, &ta, sizeof(lp::TableArgs), hipMemcpyHostToDevice, s) != hipSuccess) return LP_E_DEVICE;
        PhaseTimer T{h->tev, s};  // the column's start, rows' values, insert, index, dictionary values
        T.mark(0);
        if (lp::launch_table_values(d_args, d_targs, ta, h->d_buf, scratch, L.table_bytes, s, nullptr, false) != 0)
            return LP_E_DEVICE;
        T.mark(1);
        if (lp::launch_dict_insert(d_args, d_targs, ta, da, h->d_buf, s) != 0) return LP_E_DEVICE;
        T.mark(2);
        const uint32_t* d_total = nullptr;
        if (lp::launch_dict_rank(da, L, scratch, s, &d_total) != 0 || lp::launch_dict_index(ta, da, s) != 0) return LP_E_DEVICE;
        T.mark(3);
        uint32_t total = 0, fail = 0, bad_row = 0;
        if (!read_back(s, &total, d_total) || !read_back(s, &fail, da.fail) || (ext && !read_back(s, &bad_row, ta.bad_row)))
            return LP_E_DEVICE;
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        if (bad_row) return LP_E_INVALID;  // a rows[k] outside the batch
        if (fail) return LP_E_DEVICE;      // a probe ran out of slots
        C.dict_len = (int64_t)total;
        const bool entries_fit = C.dict_len <= C.dict_cap;
        // the dictionary's values: the STRING column of the representatives' lines (the
        // offsets into scratch when dict_off has no room: the byte total is wanted all the same)
        lp::TableArgs tv = ta;
        tv.first = 0;
        tv.count = C.dict_len;
        tv.rows = da.reps;
        tv.cols[0].valid = reinterpret_cast<uint8_t*>(da.slot);  // k_table_values writes 1 for every representative; k_table_chars reads them back
        tv.cols[0].i64 = entries_fit ? C.dict_off : const_cast<int64_t*>(da.len);
        tv.cols[0].chars = (uint8_t*)C.dict_chars;
        int64_t bytes = 0;
        if (C.dict_len == 0) {
            if (hipMemsetAsync(C.dict_off, 0, 8, s) != hipSuccess) return LP_E_DEVICE;
        } else {
            if (hipMemcpyAsync(h->targs.p, &tv, sizeof(lp::TableArgs), hipMemcpyHostToDevice, s) != hipSuccess)
                return LP_E_DEVICE;
            if (lp::launch_table_values(d_args, d_targs, tv, h->d_buf, scratch, L.table_bytes, s) != 0) return LP_E_DEVICE;
            if (!read_back(s, &bytes, tv.cols[0].i64 + C.dict_len)) return LP_E_DEVICE;
        }
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        C.dict_chars_len = (uint64_t)bytes;
        if (!entries_fit || C.dict_chars_len > C.dict_chars_cap || (bytes && !C.dict_chars)) {
            rc = LP_E_NOMEM;  // (the other columns' lengths are still set)
            continue;
        }
        if (C.dict_len > 0 && lp::launch_table_chars(d_args, d_targs, tv, h->d_buf, s) != 0) return LP_E_DEVICE;
        T.mark(4);
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        for (int k = 0; k < 4; ++k) ms[k] += T.elapsed(k, k + 1);
    }
    if (rc == LP_OK)
        for (int k = 0; k < 4; ++k) h->tms[TMS_DICT + k] = ms[k];
    return rc;
}

// rows null: row k = line first + k
static int table_dict_any(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                          lp_table_dict_col* cols, int n_cols, int threads) {
    if (!h || !r || !cols || n_cols <= 0 || count > 0x7FFFFFFF) return LP_E_INVALID;
    for (int c = 0; c < n_cols; ++c) {
        const lp_table_dict_col& C = cols[c];
        if (!C.path || !C.dict_off || C.dict_cap < 0 || (count > 0 && (!C.valid || !C.index))) return LP_E_INVALID;
    }
    for (int c = 0; c < n_cols; ++c)  // the plain STRING column of the path: its checks are this call's
        if (const int st = check_path(h, cols[c].path, LP_CAST_STRING)) return st;
    if (!r->on_host) return view_current(h, r) ? table_dict_device(h, r, first, count, rows, cols, n_cols) : LP_E_STATE;
    if (!r->input) return LP_E_INVALID;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    // a host copy: the host table's plain column, then a hash map in row order
    std::vector<lp_table_col> tc((size_t)n_cols);
    std::vector<std::vector<int64_t>> off((size_t)n_cols, std::vector<int64_t>((size_t)count + 1, 0));
    std::vector<std::vector<char>> chars((size_t)n_cols);
    uint8_t dummy_valid = 0;  // (an empty table's valid may be null)
    for (int c = 0; c < n_cols; ++c) {
        tc[c] = lp_table_col{};
        tc[c].path = cols[c].path;
        tc[c].kind = LP_CAST_STRING;
        tc[c].valid = cols[c].valid ? cols[c].valid : &dummy_valid;
        tc[c].i64 = off[c].data();
    }
    int st = table_any(h, r, first, count, rows, tc.data(), n_cols, threads);
    if (st == LP_E_NOMEM) {
        for (int c = 0; c < n_cols; ++c) {
            chars[c].resize((size_t)tc[c].chars_len + 1);
            tc[c].chars = chars[c].data();
            tc[c].chars_cap = tc[c].chars_len;
        }
        st = table_any(h, r, first, count, rows, tc.data(), n_cols, threads);
    }
    if (st != LP_OK) return st;
    int rc = LP_OK;
    for (int c = 0; c < n_cols; ++c) {
        lp_table_dict_col& C = cols[c];
        const int64_t* o = off[c].data();
        const char* b = chars[c].data();
        std::unordered_map<std::string_view, int32_t> seen;
        std::vector<int64_t> first_row;  // per entry: its first row
        std::vector<int32_t> idx((size_t)count, 0);
        uint64_t bytes = 0;
        for (int64_t k = 0; k < count; ++k) {
            if (!C.valid[k]) continue;
            const std::string_view v(b ? b + o[k] : "", (size_t)(o[k + 1] - o[k]));
            auto it = seen.find(v);
            if (it == seen.end()) {
                it = seen.emplace(v, (int32_t)first_row.size()).first;
                first_row.push_back(k);
                bytes += v.size();
            }
            idx[(size_t)k] = it->second;
        }
        C.dict_len = (int64_t)first_row.size();
        C.dict_chars_len = bytes;
        if (C.dict_len > C.dict_cap || bytes > C.dict_chars_cap || (bytes && !C.dict_chars)) {
            rc = LP_E_NOMEM;
            continue;
        }
        if (count > 0) memcpy(C.index, idx.data(), 4 * (size_t)count);
        uint64_t pos = 0;
        for (size_t j = 0; j < first_row.size(); ++j) {
            const int64_t k = first_row[j];
            C.dict_off[j] = (int64_t)pos;
            if (o[k + 1] > o[k]) memcpy(C.dict_chars + pos, b + o[k], (size_t)(o[k + 1] - o[k]));
            pos += (uint64_t)(o[k + 1] - o[k]);
        }
        C.dict_off[first_row.size()] = (int64_t)pos;
    }
    return rc;
}

int lp_result_table_dict(lp_handle* h, const lp_result* r, int64_t first, int64_t count, lp_table_dict_col* cols,
                         int n_cols, int threads) {
    return table_dict_any(h, r, first, count, nullptr, cols, n_cols, threads);
}

int lp_result_table_dict_rows(lp_handle* h, const lp_result* r, const int64_t* rows, int64_t n_rows,
                              lp_table_dict_col* cols, int n_cols, int threads) {
    return rows_arg(rows, n_rows) ? table_dict_any(h, r, 0, n_rows, rows, cols, n_cols, threads) : LP_E_INVALID;
}

// ---- wildcard targets as map columns (ParsedRecord.setMultiValueString)
namespace {
// one chunk's rows of one map column: per row its entry count, per entry the
// key / value lengths, and the bytes
struct MapChunk {
    std::vector<uint32_t> per_row, klen, vlen;
    std::string kbytes, vbytes;
};
struct MapRowCtx {
    const std::unordered_map<std::string, std::vector<int>>* by_path;
    // per column: the row's deliveries in order (key, value, live)
    struct Item {
        std::string key, val;
        bool live;
    };
    std::vector<std::vector<Item>>* items;
    std::vector<std::unordered_map<std::string, size_t>>* last;  // per column: key -> its live item
};
void map_member(void* vctx, const std::string& wildcard, const std::string& key, const lp::MVal& v) {
    MapRowCtx& t = *(MapRowCtx*)vctx;
    auto it = t.by_path->find(wildcard);
    if (it == t.by_path->end() || v.null) return;  // ParsedRecord.java:186: a null neither adds nor replaces
    for (int c : it->second) {
        auto& items = (*t.items)[c];
        auto ins = (*t.last)[c].emplace(key, items.size());
        if (!ins.second) {  // a later value of the key replaces the earlier: the entry moves here
            items[ins.first->second].live = false;
            ins.first->second = items.size();
        }
        items.push_back({key, v.is_long ? std::to_string(v.l) : std::string((const char*)v.p, v.len), true});
    }
}
}  // namespace

// lp_result_table_map / lp_result_table_map_rows on a device view: the columns
// built in HBM (table.hip).  rows as table_device's.
static int table_map_device(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                            lp_table_map_col* cols, int n_cols) {
    if (ensure_synced(h) != LP_OK) return LP_E_STATE;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    std::vector<lp::MapArgs> args((size_t)n_cols);
    for (int c = 0; c < n_cols; ++c) {
        lp::MapArgs& M = args[(size_t)c];
        memset(&M, 0, sizeof M);
        if (!h->plan.table_map_src(cols[c].path, M.src)) return LP_E_UNSUPPORTED;
        M.first = first;
        M.count = count;
        M.rows = rows;
        M.n_lines = h->n_lines;
        M.valid = cols[c].valid;
        M.entry_off = cols[c].entry_off;
        M.key_off = cols[c].key_off;
        M.val_off = cols[c].val_off;
        M.key_chars = (uint8_t*)cols[c].key_chars;
        M.val_chars = (uint8_t*)cols[c].val_chars;
    }
    hipSetDevice(h->device);
    hipStream_t s = h->stream;
    const lp::DeviceArgs* d_args = h->args.as<lp::DeviceArgs>();
    float ms[3] = {0, 0, 0};
    int rc = LP_OK;
    for (int c = 0; c < n_cols; ++c) {
        lp::MapArgs& M = args[(size_t)c];
        lp_table_map_col& C = cols[c];
        C.entries_len = C.key_chars_len = C.val_chars_len = 0;
        // the rows' piece counts and bases
        if (!h->tscratch.ensure(lp::map_scratch_bytes(count, 0))) return LP_E_NOMEM;
        const int64_t* d_total = nullptr;
        int64_t pieces = 0;
        PhaseTimer T{h->tev, s};  // start / end of the column's count, entries and fill phases
        T.mark(0);
        if (lp::launch_map_count(d_args, M, h->tscratch.p, h->tscratch.cap, s, &d_total) != 0) return LP_E_DEVICE;
        T.mark(1);
        if (!read_back(s, &pieces, d_total)) return LP_E_DEVICE;
        uint32_t bad_row = 0;  // a rows[k] outside the batch (its row: valid 0, no entries)
        if (rows && !read_back(s, &bad_row, M.bad_row)) return LP_E_DEVICE;
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        if (bad_row) return LP_E_INVALID;
        ms[0] += T.elapsed(0, 1);
        if (pieces >= 0x7FFFFFFF) return LP_E_UNSUPPORTED;  // (the scans count in ints: build it in windows)
        if (pieces == 0) {  // no entries: every row's map is empty
            if (hipMemsetAsync(C.entry_off, 0, 8 * ((size_t)count + 1), s) != hipSuccess ||
                hipMemsetAsync(C.key_off, 0, 8, s) != hipSuccess || hipMemsetAsync(C.val_off, 0, 8, s) != hipSuccess)
                return LP_E_DEVICE;
            continue;
        }
        // the surviving pieces and their byte totals
        const size_t need = lp::map_scratch_bytes(count, pieces);
        if (need > h->tscratch.cap) {  // the scratch moves: the rows' counts and bases again
            if (!h->tscratch.ensure(need)) return LP_E_NOMEM;
            if (lp::launch_map_count(d_args, M, h->tscratch.p, h->tscratch.cap, s, &d_total) != 0) return LP_E_DEVICE;
        }
        M.n_pieces = pieces;
        const void* d_tot[3] = {nullptr, nullptr, nullptr};
        uint32_t entries = 0;
        int64_t kbytes = 0, vbytes = 0;
        T.mark(2);
        if (lp::launch_map_entries(d_args, M, h->d_buf, h->tscratch.p, h->tscratch.cap, s, d_tot) != 0) return LP_E_DEVICE;
        T.mark(3);
        if (!read_back(s, &entries, d_tot[0]) || !read_back(s, &kbytes, d_tot[1]) || !read_back(s, &vbytes, d_tot[2]))
            return LP_E_DEVICE;
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        ms[1] += T.elapsed(2, 3);
        C.entries_len = entries;
        C.key_chars_len = (uint64_t)kbytes;
        C.val_chars_len = (uint64_t)vbytes;
        if (C.entries_len > C.entries_cap || C.key_chars_len > C.key_chars_cap || C.val_chars_len > C.val_chars_cap ||
            (kbytes && !C.key_chars) || (vbytes && !C.val_chars))
            rc = LP_E_NOMEM;
        if (rc != LP_OK) continue;  // (the later columns' lengths still)
        T.mark(4);
        if (lp::launch_map_fill(M, (int64_t)entries, h->tscratch.p, h->tscratch.cap, s) != 0) return LP_E_DEVICE;
        T.mark(5);
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        ms[2] += T.elapsed(4, 5);
    }
    if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
    if (rc == LP_OK)
        for (int k = 0; k < 3; ++k) h->tms[TMS_MAP + k] = ms[k];
    return rc;
}

// lp_result_table_map (rows null: row k = line first + k) and
// lp_result_table_map_rows (row k = line rows[k], first 0, count = n_rows)
static int table_map_any(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                         lp_table_map_col* cols, int n_cols, int threads) {
    if (!h || !r || !cols || n_cols <= 0) return LP_E_INVALID;
    std::unordered_map<std::string, std::vector<int>> by_path;
    for (int c = 0; c < n_cols; ++c) {  // the same validation in both modes
        const lp_table_map_col& C = cols[c];
        if (!C.path || !C.valid || !C.entry_off || !C.key_off || !C.val_off) return LP_E_INVALID;
        const std::string p = C.path;
        if (p.size() < 2 || p.compare(p.size() - 2, 2, ".*") != 0) return LP_E_INVALID;  // not a wildcard
        if (const int st = check_path(h, p, LP_CAST_STRING)) return st;  // (its wildcard request is the path itself)
        by_path[p].push_back(c);
    }
    if (!r->on_host) return view_current(h, r) ? table_map_device(h, r, first, count, rows, cols, n_cols) : LP_E_STATE;
    if (!r->input) return LP_E_INVALID;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    lp::ResultView V;
    make_view(h, *r, V);
    const Chunks ch(count, threads);
    const int T = ch.T;
    std::vector<std::vector<MapChunk>> chunk(T, std::vector<MapChunk>(n_cols));
    ch.run([&](int t, int64_t a, int64_t b) {
        std::vector<std::vector<MapRowCtx::Item>> items(n_cols);
        std::vector<std::unordered_map<std::string, size_t>> last(n_cols);
        MapRowCtx ctx{&by_path, &items, &last};
        for (int c = 0; c < n_cols; ++c) chunk[t][c].per_row.assign((size_t)(b - a), 0u);
        for (int64_t k = a; k < b; ++k) {
            const int64_t i = rows ? rows[k] : first + k;
            const bool ok = V.status && V.status[i] == LP_LINE_OK;
            for (int c = 0; c < n_cols; ++c) cols[c].valid[k] = ok ? 1 : 0;  // an OK line's record exists: its map may be empty
            if (!ok) continue;
            for (int c = 0; c < n_cols; ++c) {
                items[c].clear();
                last[c].clear();
            }
            h->plan.map_row(V, i, map_member, &ctx);
            for (int c = 0; c < n_cols; ++c) {
                MapChunk& M = chunk[t][c];
                for (const auto& it : items[c]) {
                    if (!it.live) continue;
                    ++M.per_row[(size_t)(k - a)];
                    M.klen.push_back((uint32_t)it.key.size());
                    M.vlen.push_back((uint32_t)it.val.size());
                    M.kbytes += it.key;
                    M.vbytes += it.val;
                }
            }
        }
    });
    // Arrow MapArray: row k = entries [entry_off[k], entry_off[k + 1]); entry e =
    // key_chars[key_off[e], key_off[e + 1]) -> val_chars[val_off[e], val_off[e + 1])
    int rc = LP_OK;
    for (int c = 0; c < n_cols; ++c) {
        lp_table_map_col& C = cols[c];
        uint64_t ne = 0, nk = 0, nv = 0;
        for (int t = 0; t < T; ++t) {
            ne += chunk[t][c].klen.size();
            nk += chunk[t][c].kbytes.size();
            nv += chunk[t][c].vbytes.size();
        }
        C.entries_len = ne;
        C.key_chars_len = nk;
        C.val_chars_len = nv;
        if (ne > C.entries_cap || nk > C.key_chars_cap || nv > C.val_chars_cap || (nk && !C.key_chars) ||
            (nv && !C.val_chars)) {
            rc = LP_E_NOMEM;
            continue;
        }
        uint64_t e = 0, kpos = 0, vpos = 0;
        int64_t k = 0;
        for (int t = 0; t < T; ++t) {
            const MapChunk& M = chunk[t][c];
            for (uint32_t n : M.per_row) {
                C.entry_off[k++] = (int64_t)e;
                e += n;
            }
            uint64_t kp = kpos, vp = vpos, e0 = e - M.klen.size();
            for (size_t q = 0; q < M.klen.size(); ++q) {
                C.key_off[e0 + q] = (int64_t)kp;
                C.val_off[e0 + q] = (int64_t)vp;
                kp += M.klen[q];
                vp += M.vlen[q];
            }
            if (!M.kbytes.empty()) memcpy(C.key_chars + kpos, M.kbytes.data(), M.kbytes.size());
            if (!M.vbytes.empty()) memcpy(C.val_chars + vpos, M.vbytes.data(), M.vbytes.size());
            kpos = kp;
            vpos = vp;
        }
        C.entry_off[count] = (int64_t)e;
        C.key_off[e] = (int64_t)kpos;
        C.val_off[e] = (int64_t)vpos;
    }
    return rc;
}

int lp_result_table_map(lp_handle* h, const lp_result* r, int64_t first, int64_t count, lp_table_map_col* cols, int n_cols,
                        int threads) {
    return table_map_any(h, r, first, count, nullptr, cols, n_cols, threads);
}

int lp_result_table_map_rows(lp_handle* h, const lp_result* r, const int64_t* rows, int64_t n_rows, lp_table_map_col* cols,
                             int n_cols, int threads) {
    return rows_arg(rows, n_rows) ? table_map_any(h, r, 0, n_rows, rows, cols, n_cols, threads) : LP_E_INVALID;
}

// ---- row selection: lp_result_select and lp_result_select_where, one implementation
namespace {
// a term's value on a host copy, as table_value leaves it in the term's column: 0 null, 1 bytes, 2 a long
struct WhereVal {
    int kind = 0;
    std::string s;
    int64_t l = 0;
};
struct WhereCtx {
    const std::unordered_map<std::string, std::vector<int>>* by_path;
    const lp_where_term* terms;
    WhereVal* vals;
};
// ParsedRecord.set as table_value does it: a null is ignored, the last value wins; a LONG column keeps
// its earlier value when the later one does not parse
void where_value(void* vctx, const std::string& target, const lp::MVal& v) {
    WhereCtx& w = *(WhereCtx*)vctx;
    auto it = w.by_path->find(target);
    if (it == w.by_path->end() || v.null) return;
    for (int t : it->second) {
        WhereVal& x = w.vals[t];
        if (v.is_long) {
            x.kind = 2;
            x.l = v.l;
        } else if (w.terms[t].kind == LP_CAST_STRING) {
            x.kind = 1;
            x.s.assign((const char*)v.p, v.len);
        } else if (java_parse_long(v.p, v.len, x.l)) {
            x.kind = 2;
        }
    }
}
// the term's rule (lp_pred.h) on such a value
bool where_term(const lp_where_term& t, const WhereVal& x) {
    if (t.kind == LP_CAST_LONG) return lp::pred_term_long(t.op, x.kind == 0, x.l, t.lo, t.hi);
    if (x.kind == 2) {  // a STRING taken from a long: its decimal text
        char b[20];
        const uint32_t n = lp::digits(x.l);
        lp::write_long(b, x.l, n);
        lp::PredLocal v{b, n};
        return lp::pred_term_bytes(t.op, false, v, t.str, (uint32_t)t.str_len);
    }
    lp::PredBytes<const uint8_t*> v{(const uint8_t*)x.s.data(), (uint32_t)x.s.size(), false};
    return lp::pred_term_bytes(t.op, x.kind == 0, v, t.str, (uint32_t)t.str_len);
}
}  // namespace

// The terms of a lp_result_select_where call, in both modes: pseudo[t] the
// term's TC_* kind when its path is a pseudo-column
static int check_terms(lp_handle* h, const lp_where_term* terms, int n_terms, std::vector<int>& pseudo) {
    if (n_terms < 0 || n_terms > LP_WHERE_MAX_TERMS || (n_terms > 0 && !terms)) return LP_E_INVALID;
    pseudo.assign((size_t)n_terms, 0);
    for (int t = 0; t < n_terms; ++t) {
        const lp_where_term& W = terms[t];
        if (!W.path || (W.kind != LP_CAST_STRING && W.kind != LP_CAST_LONG)) return LP_E_INVALID;
        if (!lp::pred_op_ok(W.op, W.kind == LP_CAST_STRING ? 1 : 2)) return LP_E_INVALID;
        if (t > 0 && W.group < terms[t - 1].group) return LP_E_INVALID;
        if (W.str_len < 0 || W.str_len > lp::PRED_MAX_STR || (W.str_len > 0 && !W.str)) return LP_E_INVALID;
        if (const int st = check_path(h, W.path, W.kind, &pseudo[t])) return st;
    }
    return LP_OK;
}

// The terms bound for k_where_eval: column t of ta is term t's (Plan::table_src),
// the STRING operands follow the names in ta's pool
static int bind_terms(lp_handle* h, const lp_where_term* terms, int n_terms, lp::TableArgs& ta, lp::WhereArgs& wa) {
    std::string names;
    size_t operands = 0;
    for (int t = 0; t < n_terms; ++t) operands += terms[t].kind == LP_CAST_STRING ? (size_t)terms[t].str_len : 0;
    for (int t = 0; t < n_terms; ++t) {
        lp::TableCol& T = ta.cols[t];
        T.kind = terms[t].kind;
        const std::string path = terms[t].path;
        if (!h->plan.table_src(path, T.src, names, T.alt))  // (false also when the names pool is full)
            return names.size() + path.size() + operands > (size_t)lp::TABLE_NAMES ? LP_E_INVALID : LP_E_UNSUPPORTED;
    }
    if (names.size() + operands > (size_t)lp::TABLE_NAMES) return LP_E_INVALID;
    for (int t = 0; t < n_terms; ++t) {
        lp::WhereTerm& R = wa.t[t];
        R.op = terms[t].op;
        R.group = terms[t].group;
        R.lo = terms[t].lo;
        R.hi = terms[t].hi;
        R.str_off = (int32_t)names.size();
        R.str_len = terms[t].kind == LP_CAST_STRING ? terms[t].str_len : 0;
        if (R.str_len > 0) names.append((const char*)terms[t].str, (size_t)R.str_len);
    }
    memcpy(ta.names, names.data(), names.size());
    wa.n_terms = n_terms;
    return LP_OK;
}

// The lines of a window whose status is in status_mask -- and on which the
// terms' predicate holds -- ascending.  A device view: select.hip's stream
// compaction of the status column, or (terms) of the bits where.hip's
// k_where_eval leaves; a host copy: a loop over the copied status column and
// (terms) the host replay's values.
static int select_any(lp_handle* h, const lp_result* r, int64_t first, int64_t count, uint32_t status_mask,
                      const lp_where_term* terms, int n_terms, int64_t* rows, uint64_t rows_cap, uint64_t* rows_len) {
    if (!h || !r || !rows_len) return LP_E_INVALID;
    if (status_mask & ~(uint32_t)(LP_SEL_OK | LP_SEL_BAD | LP_SEL_FALLBACK)) return LP_E_INVALID;
    *rows_len = 0;
    std::vector<int> pseudo;
    if (const int st = check_terms(h, terms, n_terms, pseudo)) return st;
    if (!r->on_host) {
        if (!view_current(h, r) || ensure_synced(h) != LP_OK) return LP_E_STATE;
        if (!check_window(first, count, nullptr, h->n_lines)) return LP_E_INVALID;
        if (rows_cap && !device_memory(h, rows)) return LP_E_INVALID;
        std::unique_ptr<lp::TableArgs> ta;
        lp::WhereArgs wa{};
        if (n_terms > 0) {
            ta = table_args(h, 0, 0, nullptr, n_terms);
            if (const int st = bind_terms(h, terms, n_terms, *ta, wa)) return st;
        }
        if (count == 0 || status_mask == 0) return LP_OK;
        hipSetDevice(h->device);
        hipStream_t s = h->stream;
        if (!h->tscratch.ensure(lp::select_scratch_bytes(first, count))) return LP_E_NOMEM;
        const bool where = n_terms > 0;
        PhaseTimer T{h->tev, s};  // start, (terms: the predicate kernel done,) end of the compaction
        if (where) {
            if (!h->targs.ensure(sizeof(lp::TableArgs))) return LP_E_NOMEM;
            if (hipMemcpyAsync(h->targs.p, ta.get(), sizeof(lp::TableArgs), hipMemcpyHostToDevice, s) != hipSuccess)
                return LP_E_DEVICE;
            wa.first = first;
            wa.count = count;
            wa.mask = status_mask;
            wa.bits = lp::select_bits(first, count, h->tscratch.p, h->tscratch.cap);
            T.mark(2);
            if (lp::launch_where_eval(h->args.as<lp::DeviceArgs>(), h->targs.as<lp::TableArgs>(), *ta, h->d_buf, wa, s) != 0)
                return LP_E_DEVICE;
        }
        const int64_t* d_total = nullptr;
        int64_t total = 0;
        T.mark(0);
        if (lp::launch_select_count(h->C.status, first, count, status_mask, h->tscratch.p, h->tscratch.cap, s, &d_total,
                                    where) != 0)
            return LP_E_DEVICE;
        // the number of selected lines decides whether they fit
        if (!read_back(s, &total, d_total)) return LP_E_DEVICE;
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        *rows_len = (uint64_t)total;
        if ((uint64_t)total > rows_cap) return LP_E_NOMEM;
        if (total > 0 && lp::launch_select_write(h->C.status, first, count, status_mask, rows, h->tscratch.p,
                                                 h->tscratch.cap, s, where) != 0)
            return LP_E_DEVICE;
        T.mark(1);
        if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
        // (the host's read of the total between the passes is inside the interval)
        if (where) {
            h->tms[TMS_WHERE] = T.elapsed(2, 0);
            h->tms[TMS_WHERE + 1] = T.elapsed(0, 1);
        } else {
            h->tms[TMS_SELECT] = T.elapsed(0, 1);
        }
        return LP_OK;
    }
    if (n_terms > 0 && !r->input) return LP_E_INVALID;  // (the values are read from the copied input)
    if (n_terms > 0) {  // the names pool's bound holds in both modes (what only the device refuses does not)
        auto ta = table_args(h, 0, 0, nullptr, n_terms);
        lp::WhereArgs wa{};
        if (bind_terms(h, terms, n_terms, *ta, wa) == LP_E_INVALID) return LP_E_INVALID;
    }
    if (!check_window(first, count, nullptr, r->n_lines)) return LP_E_INVALID;
    lp::ResultView V;
    make_view(h, *r, V);
    if (!V.status && count > 0) return LP_E_INVALID;
    std::unordered_map<std::string, std::vector<int>> by_path;
    for (int t = 0; t < n_terms; ++t)
        if (!pseudo[t]) by_path[terms[t].path].push_back(t);
    std::vector<WhereVal> vals((size_t)n_terms);
    auto selected = [&](int64_t i) {
        const uint32_t st = V.status[i];
        if (((status_mask >> (st & 7u)) & 1u) == 0) return false;
        if (n_terms == 0) return true;
        for (auto& x : vals) x.kind = 0;
        if (st == LP_LINE_OK && !by_path.empty()) {
            WhereCtx ctx{&by_path, terms, vals.data()};
            h->plan.rec_row(V, i, where_value, &ctx);
        }
        lp::PredFold F;
        for (int t = 0; t < n_terms; ++t) {
            lp::pred_fold_group(F, t, terms[t].group);
            if (!lp::pred_fold_wants(F)) continue;
            bool out;
            if (pseudo[t] == lp::TC_LINE) {  // the line as the parse kernels see it (kernels_common.h crlf_len)
                const uint64_t s0 = V.line_off[i];
                uint64_t n = V.line_off[i + 1] - 1 - s0;
                if (n > 0 && V.input[s0 + n - 1] == '\r') --n;
                lp::PredBytes<const uint8_t*> v{V.input + s0, (uint32_t)n, false};
                out = lp::pred_term_bytes(terms[t].op, false, v, terms[t].str, (uint32_t)terms[t].str_len);
            } else if (pseudo[t]) {
                const int64_t x = pseudo[t] == lp::TC_OFFSET ? (int64_t)V.line_off[i]
                                  : pseudo[t] == lp::TC_LINENO ? r->first_line + i : (int64_t)st;
                out = lp::pred_term_long(terms[t].op, false, x, terms[t].lo, terms[t].hi);
            } else {
                out = where_term(terms[t], vals[(size_t)t]);
            }
            lp::pred_fold_term(F, out);
        }
        return lp::pred_fold_result(F, n_terms);
    };
    // (one evaluation per line: the matches, then whether they fit)
    std::vector<int64_t> got;
    for (int64_t i = first; i < first + count; ++i)
        if (selected(i)) got.push_back(i);
    *rows_len = (uint64_t)got.size();
    if (got.size() > rows_cap || (!got.empty() && !rows)) return LP_E_NOMEM;  // (nothing written)
    if (!got.empty()) memcpy(rows, got.data(), 8 * got.size());
    return LP_OK;
}

int lp_result_select(lp_handle* h, const lp_result* r, int64_t first, int64_t count, uint32_t status_mask, int64_t* rows,
                     uint64_t rows_cap, uint64_t* rows_len) {
    return select_any(h, r, first, count, status_mask, nullptr, 0, rows, rows_cap, rows_len);
}

int lp_result_select_where(lp_handle* h, const lp_result* r, int64_t first, int64_t count, uint32_t status_mask,
                           const lp_where_term* terms, int n_terms, int64_t* rows, uint64_t rows_cap, uint64_t* rows_len) {
    return select_any(h, r, first, count, status_mask, terms, n_terms, rows, rows_cap, rows_len);
}

// ---- grouped aggregates (GROUP BY): lp_result_group / lp_result_group_rows
namespace {
// the checked arguments of a call, in both modes: the distinct measure paths in the order of
// their first aggregate, and the accumulator words (lp_group.h)
struct GroupSpec {
    std::vector<std::string> meas;
    lp::GroupAccs A{};
};
}  // namespace

static int check_group(lp_handle* h, int64_t count, const lp_group_key* keys, int n_keys, const lp_group_agg* aggs,
                       int n_aggs, lp_group_out* out, GroupSpec& S) {
    if (n_keys < 0 || n_keys > LP_GROUP_MAX_KEYS || (n_keys > 0 && !keys)) return LP_E_INVALID;
    if (n_aggs < 0 || n_aggs > LP_GROUP_MAX_AGGS || (n_aggs > 0 && !aggs)) return LP_E_INVALID;
    if (out->groups_cap < 0 || (out->groups_cap > 0 && !out->rep) || count > 0x7FFFFFFF) return LP_E_INVALID;
    for (int c = 0; c < n_keys; ++c)
        if (!keys[c].path || (keys[c].kind != LP_CAST_STRING && keys[c].kind != LP_CAST_LONG)) return LP_E_INVALID;
    int32_t op[LP_GROUP_MAX_AGGS], meas[LP_GROUP_MAX_AGGS];
    for (int a = 0; a < n_aggs; ++a) {
        const lp_group_agg& G = aggs[a];
        if (G.op < LP_AGG_COUNT_ROWS || G.op > LP_AGG_MAX || (G.op == LP_AGG_COUNT_ROWS) != (G.path == nullptr))
            return LP_E_INVALID;
        if (out->groups_cap > 0 && (!G.value || !G.valid)) return LP_E_INVALID;
        op[a] = G.op;
        meas[a] = -1;
        if (!G.path) continue;
        const auto it = std::find(S.meas.begin(), S.meas.end(), G.path);
        meas[a] = (int32_t)(it - S.meas.begin());
        if (it == S.meas.end()) S.meas.push_back(G.path);
    }
    for (int c = 0; c < n_keys; ++c)
        if (const int st = check_path(h, keys[c].path, keys[c].kind)) return st;
    for (const std::string& p : S.meas)
        if (const int st = check_path(h, p, LP_CAST_LONG)) return st;
    S.A = lp::group_accs(n_aggs, op, meas, (int)S.meas.size());
    return LP_OK;
}

// On a device view (group.hip; kernels.h GroupLayout): the keys' hash and the
// insert, the dictionary's numbering, then -- the groups counted and found to
// fit -- the accumulation.
static int group_device(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                        const lp_group_key* keys, int n_keys, const lp_group_agg* aggs, int n_aggs, lp_group_out* out,
                        const GroupSpec& S) {
    if (ensure_synced(h) != LP_OK) return LP_E_STATE;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    if (out->groups_cap > 0) {  // every array the kernels write is memory of the device
        if (!device_memory(h, out->rep)) return LP_E_INVALID;
        for (int a = 0; a < n_aggs; ++a)
            if (!device_memory(h, aggs[a].value) || !device_memory(h, aggs[a].valid)) return LP_E_INVALID;
    }
    if (count > 0 && out->group_of && !device_memory(h, out->group_of)) return LP_E_INVALID;
    const int n_meas = (int)S.meas.size();
    auto ta = table_args(h, first, count, rows, n_keys + n_meas);
    std::string names;
    for (int c = 0; c < n_keys + n_meas; ++c) {
        lp::TableCol& T = ta->cols[c];
        const std::string path = c < n_keys ? keys[c].path : S.meas[(size_t)(c - n_keys)];
        T.kind = c < n_keys ? keys[c].kind : LP_CAST_LONG;
        if (!h->plan.table_src(path, T.src, names, T.alt))  // (false also when the names pool is full)
            return names.size() + path.size() > (size_t)lp::TABLE_NAMES ? LP_E_INVALID : LP_E_UNSUPPORTED;
    }
    memcpy(ta->names, names.data(), names.size());
    if (count == 0) return LP_OK;  // (no launch, no event: lp_last_timing [20..22] keep the last call's)
    hipSetDevice(h->device);
    hipStream_t s = h->stream;
    if (!h->targs.ensure(sizeof(lp::TableArgs))) return LP_E_NOMEM;
    const lp::GroupLayout L = lp::group_layout(count);
    if (!h->tscratch.ensure(L.total)) return LP_E_NOMEM;
    lp::GroupArgs ga{};
    lp::DictArgs da{};
    ga.count = da.count = count;
    ga.n_keys = n_keys;
    ga.hash_bits = h->dict_hash_bits;
    ga.peel = h->group_peel < 0 ? 0 : h->group_peel == 0 ? lp::GROUP_PEEL_ROUNDS : h->group_peel;
    ga.A = S.A;
    lp::group_bind(ga, da, *ta, L, h->tscratch.p, out->group_of);
    if (hipMemcpyAsync(h->targs.p, ta.get(), sizeof(lp::TableArgs), hipMemcpyHostToDevice, s) != hipSuccess) return LP_E_DEVICE;
    const lp::DeviceArgs* d_args = h->args.as<lp::DeviceArgs>();
    const lp::TableArgs* d_targs = h->targs.as<lp::TableArgs>();
    PhaseTimer T{h->tev, s};  // start, insert done, numbering done, aggregation done
    T.mark(0);
    if (lp::launch_group_insert(d_args, d_targs, *ta, ga, h->d_buf, s) != 0) return LP_E_DEVICE;
    T.mark(1);
    const uint32_t* d_total = nullptr;
    if (lp::launch_dict_rank(da, L.d, h->tscratch.p, s, &d_total) != 0 || lp::launch_dict_index(*ta, da, s) != 0)
        return LP_E_DEVICE;
    T.mark(2);
    uint32_t total = 0, fail = 0, bad_row = 0;
    if (!read_back(s, &total, d_total) || !read_back(s, &fail, da.fail) || !read_back(s, &bad_row, ta->bad_row))
        return LP_E_DEVICE;
    if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
    if (bad_row) return LP_E_INVALID;  // a rows[k] outside the batch
    if (fail) return LP_E_DEVICE;      // a probe ran out of slots
    out->n_groups = (int64_t)total;
    if (out->n_groups > out->groups_cap) return LP_E_NOMEM;
    if (!h->gacc.ensure(8 * (size_t)total * (size_t)S.A.n_words)) return LP_E_NOMEM;
    ga.n_groups = out->n_groups;
    ga.acc = h->gacc.as<int64_t>();
    if (hipMemcpyAsync(out->rep, (const void*)da.reps, 8 * (size_t)total, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return LP_E_DEVICE;
    const int64_t budget = h->group_lds_words < 0 ? 0 : h->group_lds_words == 0 ? lp::GROUP_LDS_WORDS : h->group_lds_words;
    if (lp::launch_group_agg(d_args, d_targs, *ta, ga, h->d_buf, budget, s, nullptr) != 0) return LP_E_DEVICE;
    lp::GroupOut go{};
    go.groups = out->n_groups;
    for (int a = 0; a < n_aggs; ++a) {
        go.value[a] = aggs[a].value;
        go.valid[a] = aggs[a].valid;
    }
    if (lp::launch_group_finish(ga, go, s) != 0) return LP_E_DEVICE;
    T.mark(3);
    if (hipStreamSynchronize(s) != hipSuccess) return LP_E_DEVICE;
    for (int k = 0; k < 3; ++k) h->tms[TMS_GROUP + k] = T.elapsed(k, k + 1);
    return LP_OK;
}

// rows null: row k = line first + k
static int group_any(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const int64_t* rows,
                     const lp_group_key* keys, int n_keys, const lp_group_agg* aggs, int n_aggs, lp_group_out* out,
                     int threads) {
    if (!h || !r || !out) return LP_E_INVALID;
    out->n_groups = 0;
    GroupSpec S;
    if (const int st = check_group(h, count, keys, n_keys, aggs, n_aggs, out, S)) return st;
    if (!r->on_host)
        return view_current(h, r) ? group_device(h, r, first, count, rows, keys, n_keys, aggs, n_aggs, out, S) : LP_E_STATE;
    if (!r->input) return LP_E_INVALID;
    if (const int st = check_rows(h, r, first, count, rows)) return st;
    if (count == 0) return LP_OK;
    // a host copy: the host table's columns of the keys and the distinct measures, then a hash map in row order
    const int n_meas = (int)S.meas.size(), n_cols = n_keys + n_meas;
    std::vector<lp_table_col> tc((size_t)n_cols);
    std::vector<std::vector<uint8_t>> valid((size_t)n_cols, std::vector<uint8_t>((size_t)count, 0));
    std::vector<std::vector<int64_t>> i64((size_t)n_cols, std::vector<int64_t>((size_t)count + 1, 0));
    std::vector<std::vector<char>> chars((size_t)n_cols);
    for (int c = 0; c < n_cols; ++c) {
        tc[c] = lp_table_col{};
        tc[c].path = c < n_keys ? keys[c].path : S.meas[(size_t)(c - n_keys)].c_str();
        tc[c].kind = c < n_keys ? keys[c].kind : LP_CAST_LONG;
        tc[c].valid = valid[c].data();
        tc[c].i64 = i64[c].data();
    }
    if (n_cols > 0) {
        int st = table_any(h, r, first, count, rows, tc.data(), n_cols, threads);
        if (st == LP_E_NOMEM) {
            for (int c = 0; c < n_cols; ++c) {
                chars[c].resize((size_t)tc[c].chars_len + 1);
                tc[c].chars = chars[c].data();
                tc[c].chars_cap = tc[c].chars_len;
            }
            st = table_any(h, r, first, count, rows, tc.data(), n_cols, threads);
        }
        if (st != LP_OK) return st;
    }
    const lp::GroupAccs& A = S.A;
    const int W = A.n_words;
    std::unordered_map<std::string, int32_t> seen;
    std::vector<int64_t> reps, acc;
    std::vector<int32_t> group_of((size_t)count, 0);
    std::string key;
    for (int64_t k = 0; k < count; ++k) {
        key.clear();  // per key: a null tag, then the int64 or the length and the bytes
        for (int c = 0; c < n_keys; ++c) {
            key.push_back(valid[c][(size_t)k] ? 1 : 0);
            if (!valid[c][(size_t)k]) continue;
            if (keys[c].kind == LP_CAST_LONG) {
                key.append((const char*)&i64[c][(size_t)k], 8);
            } else {
                const int64_t n = i64[c][(size_t)k + 1] - i64[c][(size_t)k];
                key.append((const char*)&n, 8);
                if (n > 0) key.append(chars[c].data() + i64[c][(size_t)k], (size_t)n);
            }
        }
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int32_t)reps.size()).first;
            reps.push_back(rows ? rows[k] : first + k);
            for (int w = 0; w < W; ++w) acc.push_back(lp::group_identity(A.wkind[w]));
        }
        const int32_t g = it->second;
        group_of[(size_t)k] = g;
        int64_t* w = acc.data() + (size_t)g * (size_t)W;
        for (int x = 0; x < W; ++x) {
            const int m = A.wmeas[x];
            const bool ok = m >= 0 && valid[n_keys + m][(size_t)k];
            w[x] = lp::group_merge(A.wkind[x], w[x], lp::group_contrib(A.wkind[x], ok, ok ? i64[n_keys + m][(size_t)k] : 0));
        }
    }
    out->n_groups = (int64_t)reps.size();
    if (out->n_groups > out->groups_cap) return LP_E_NOMEM;  // (nothing written)
    memcpy(out->rep, reps.data(), 8 * reps.size());
    if (out->group_of) memcpy(out->group_of, group_of.data(), 4 * (size_t)count);
    for (int64_t g = 0; g < out->n_groups; ++g)
        for (int a = 0; a < n_aggs; ++a)
            aggs[a].value[g] = lp::group_value(A, a, acc.data() + (size_t)g * (size_t)W, aggs[a].valid[g]);
    return LP_OK;
}

int lp_result_group(lp_handle* h, const lp_result* r, int64_t first, int64_t count, const lp_group_key* keys, int n_keys,
                    const lp_group_agg* aggs, int n_aggs, lp_group_out* out, int threads) {
    return group_any(h, r, first, count, nullptr, keys, n_keys, aggs, n_aggs, out, threads);
}

int lp_result_group_rows(lp_handle* h, const lp_result* r, const int64_t* rows, int64_t n_rows, const lp_group_key* keys,
                         int n_keys, const lp_group_agg* aggs, int n_aggs, lp_group_out* out, int threads) {
    return rows_arg(rows, n_rows) ? group_any(h, r, 0, n_rows, rows, keys, n_keys, aggs, n_aggs, out, threads) : LP_E_INVALID;
}

// ---- Arrow C Data Interface export (arrow_export.cpp, lp_arrow.h)
namespace {
// Every buffer of one exported batch (malloc on a host copy, hipMalloc on a
// device view): the context of the owner the packaging calls when the
// consumer has released the batch's last structure
struct ArrowBufs {
    bool host = true;
    std::vector<void*> p;
    void* get(size_t bytes) {
        void* q = nullptr;
        if (bytes == 0) bytes = 64;  // (never a null buffer, even without elements)
        if (host) q = malloc(bytes);
        else if (hipMalloc(&q, bytes) != hipSuccess) q = nullptr;
        if (q) p.push_back(q);
        return q;
    }
    ~ArrowBufs() {
        for (void* q : p) {
            if (host) free(q);
            else (void)hipFree(q);
        }
    }
};
void arrow_bufs_free(void* ctx) { delete static_cast<ArrowBufs*>(ctx); }

// A table family's call with its size protocol: after LP_E_NOMEM grow() makes
// what the reported lengths ask for (false: no memory) and the call runs once more
int arrow_sized(const std::function<int()>& call, const std::function<bool()>& grow) {
    int st = call();
    if (st == LP_E_NOMEM) st = grow() ? call() : LP_E_NOMEM;
    return st;
}
}  // namespace

static int result_arrow(lp_handle* h, const lp_result* r, const int64_t* rows, int64_t first, int64_t count,
                        const lp_arrow_col* cols, int n_cols, int threads, ArrowSchema* schema_out,
                        ArrowDeviceArray* array_out) {
    if (!h || !r || !cols || n_cols <= 0 || !schema_out || !array_out) return LP_E_INVALID;
    if (rows) {
        first = 0;
        if (!rows_arg(rows, count)) return LP_E_INVALID;
    }
    // (the table calls check the window again; here it bounds what is allocated)
    if (count < 0 || ((r->on_host || view_current(h, r)) && !check_window(first, count, rows, r->on_host ? r->n_lines : h->n_lines)))
        return LP_E_INVALID;
    // the columns by family, and where each stands in the batch
    std::vector<lp_table_col> P;
    std::vector<lp_table_dict_col> D;
    std::vector<lp_table_map_col> M;
    std::vector<const char*> pn, dn, mn;
    std::vector<int> slot((size_t)n_cols);
    for (int c = 0; c < n_cols; ++c) {
        const lp_arrow_col& A = cols[c];
        if (!A.path) return LP_E_INVALID;
        if (A.form == LP_ARROW_PLAIN) {
            lp_table_col t{};
            t.path = A.path;
            t.kind = A.kind;
            slot[(size_t)c] = (int)P.size();
            P.push_back(t);
            pn.push_back(A.name);
        } else if (A.form == LP_ARROW_DICT) {
            lp_table_dict_col t{};
            t.path = A.path;
            slot[(size_t)c] = (int)D.size();
            D.push_back(t);
            dn.push_back(A.name);
        } else if (A.form == LP_ARROW_MAP) {
            lp_table_map_col t{};
            t.path = A.path;
            slot[(size_t)c] = (int)M.size();
            M.push_back(t);
            mn.push_back(A.name);
        } else {
            return LP_E_INVALID;
        }
    }
    const int nP = (int)P.size(), nD = (int)D.size(), nM = (int)M.size();
    std::vector<int> order((size_t)n_cols);
    for (int c = 0; c < n_cols; ++c)
        order[(size_t)c] = slot[(size_t)c] + (cols[c].form == LP_ARROW_PLAIN ? 0 : cols[c].form == LP_ARROW_DICT ? nP : nP + nD);
    const bool host = r->on_host != 0;
    auto B = std::make_unique<ArrowBufs>();
    B->host = host;
    if (!host) hipSetDevice(h->device);
    const size_t n1 = (size_t)count;
    bool mem = true;
    auto get = [&](auto*& dst, size_t bytes) {
        dst = static_cast<std::remove_reference_t<decltype(dst)>>(B->get(bytes));
        if (!dst) mem = false;
    };
    for (lp_table_col& C : P) {
        get(C.valid, n1);
        if (C.kind == LP_CAST_DOUBLE) get(C.f64, 8 * n1);
        else get(C.i64, 8 * (n1 + 1));
    }
    for (lp_table_dict_col& C : D) {
        get(C.valid, n1);
        get(C.index, 4 * n1);
        get(C.dict_off, 8);
    }
    for (lp_table_map_col& C : M) {
        get(C.valid, n1);
        get(C.entry_off, 8 * (n1 + 1));
        get(C.key_off, 8);
        get(C.val_off, 8);
    }
    if (!mem) return LP_E_NOMEM;
    // the tables' own paths fill them: their checks, their codes, their size protocol
    if (nP) {
        const int st = arrow_sized([&] { return table_any(h, r, first, count, rows, P.data(), nP, threads); },
                                   [&] {
                                       for (lp_table_col& C : P)
                                           if (C.kind == LP_CAST_STRING && C.chars_len > C.chars_cap) {
                                               get(C.chars, (size_t)C.chars_len);
                                               C.chars_cap = C.chars_len;
                                           }
                                       return mem;
                                   });
        if (st != LP_OK) return st;
        for (lp_table_col& C : P)
            if (C.kind == LP_CAST_STRING && !C.chars) get(C.chars, 0);
    }
    if (nD) {
        const int st = arrow_sized([&] { return table_dict_any(h, r, first, count, rows, D.data(), nD, threads); },
                                   [&] {
                                       for (lp_table_dict_col& C : D) {
                                           if (C.dict_len > C.dict_cap) {
                                               get(C.dict_off, 8 * ((size_t)C.dict_len + 1));
                                               C.dict_cap = C.dict_len;
                                           }
                                           if (C.dict_chars_len > C.dict_chars_cap) {
                                               get(C.dict_chars, (size_t)C.dict_chars_len);
                                               C.dict_chars_cap = C.dict_chars_len;
                                           }
                                       }
                                       return mem;
                                   });
        if (st != LP_OK) return st;
        for (lp_table_dict_col& C : D)
            if (!C.dict_chars) get(C.dict_chars, 0);
    }
    if (nM) {
        bool too_long = false;  // Arrow's map has int32 offsets
        const int st = arrow_sized([&] { return table_map_any(h, r, first, count, rows, M.data(), nM, threads); },
                                   [&] {
                                       for (lp_table_map_col& C : M) {
                                           if (C.entries_len > 0x7FFFFFFFull) return !(too_long = true);
                                           if (C.entries_len > C.entries_cap) {
                                               get(C.key_off, 8 * ((size_t)C.entries_len + 1));
                                               get(C.val_off, 8 * ((size_t)C.entries_len + 1));
                                               C.entries_cap = C.entries_len;
                                           }
                                           if (C.key_chars_len > C.key_chars_cap) {
                                               get(C.key_chars, (size_t)C.key_chars_len);
                                               C.key_chars_cap = C.key_chars_len;
                                           }
                                           if (C.val_chars_len > C.val_chars_cap) {
                                               get(C.val_chars, (size_t)C.val_chars_len);
                                               C.val_chars_cap = C.val_chars_len;
                                           }
                                       }
                                       return mem;
                                   });
        if (too_long) return LP_E_INVALID;
        if (st != LP_OK) return st;
        for (lp_table_map_col& C : M) {
            if (!C.key_chars) get(C.key_chars, 0);
            if (!C.val_chars) get(C.val_chars, 0);
        }
    }
    if (!mem) return LP_E_NOMEM;
    // the packaging wraps them; the owner frees them when the consumer is done
    const lp_arrow_owner owner{arrow_bufs_free, B.get()};
    float ms = 0;
    const int st = lp::arrow_wrap(host ? -1 : h->device, h->stream, count, P.data(), pn.data(), nP, D.data(), dn.data(), nD,
                                  M.data(), mn.data(), nM, order.data(), &owner, schema_out, array_out, host ? nullptr : &ms);
    if (st != LP_OK) return st;  // (the owner was not called: B frees the buffers)
    B.release();
    if (!host && count > 0) h->tms[TMS_ARROW] = ms;  // (an empty export launches no bitmap kernel and keeps the last figure)
    return LP_OK;
}

int lp_result_arrow(lp_handle* h, const lp_result* r, const int64_t* rows, int64_t first, int64_t count,
                    const lp_arrow_col* cols, int n_cols, int threads, ArrowSchema* schema_out,
                    ArrowDeviceArray* array_out) {
    if (schema_out) memset(schema_out, 0, sizeof *schema_out);
    if (array_out) memset(array_out, 0, sizeof *array_out);
    try {
        return result_arrow(h, r, rows, first, count, cols, n_cols, threads, schema_out, array_out);
    } catch (const std::bad_alloc&) {
        return LP_E_NOMEM;
    }
}

int lp_result_emit(lp_handle* h, const lp_result* r, int64_t i, lp_emit_fn fn, void* ctx) {
    if (!h || !r || !fn || !r->on_host || !r->input) return LP_E_INVALID;
    if (i < 0 || i >= r->n_lines) return LP_E_INVALID;
    lp::ResultView V;
    make_view(h, *r, V);
    if (!V.status || V.status[i] != LP_LINE_OK) return LP_E_STATE;
    return h->plan.emit_row(V, i, fn, ctx);
}

}  // extern "C"
