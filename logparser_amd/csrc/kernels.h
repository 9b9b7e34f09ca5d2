// Host-callable launchers of the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "lp_group.h"
#include "lp_program.h"
#include "lp_table.h"

namespace lp {

// Everything the parse kernels read besides the input: copied to the device
// per batch (stream-ordered), so concurrent handles never share state.
struct DeviceArgs {
    Program prog;
    Columns cols;
};

int64_t count_chunks(uint64_t nbytes);
inline int64_t nlmask_words(uint64_t nbytes) { return count_chunks(nbytes) * (64 * 1024 / 16); }
// line index, pass 1: per-chunk '\n' counts (exclusively scanned in place,
// d_chunk needs count_chunks()+1 entries) and the '\n' bit mask of every 16
// input bytes (d_nlmask, nlmask_words() entries); the scan also sets
// meta->n_lines (Hadoop LineRecordReader count: a final unterminated line
// counts), line_off[0] and the end sentinel, and meta->cap_ovf when the
// batch has more lines than the columns hold (cap_lines).
int launch_count(const uint8_t* d_buf, uint64_t nbytes, uint64_t* d_chunk, uint16_t* d_nlmask, uint64_t* d_line_off,
                 int64_t cap_lines, Meta* d_meta, hipStream_t s);
// line index, pass 2 (from the masks): line_off[k] = start of line k (k <= cap_lines)
int launch_offsets(const uint16_t* d_nlmask, uint64_t nbytes, const uint64_t* d_chunk, uint64_t* d_line_off,
                   int64_t cap_lines, hipStream_t s);

// parse kernels: one wave per 64 lines (C.wave_counts needs WC_WORDS u32 per wave)
constexpr int WC_WORDS = 8;
int64_t parse_waves(int64_t n_lines);
struct ParseLaunch {
    const uint8_t* buf;
    uint64_t nbytes;
    int64_t cap_lines;      // grid: parse_waves(cap_lines) waves; lines >= meta->n_lines exit
    uint64_t mean_line;     // expected mean line length (sizes the LDS window)
    int n_elems, stack_depth;
    bool force_direct;      // every wave on the direct (HBM) path: tests / diagnostics only
    bool uri;               // the program has URI stages (k_uri_lines after the parse kernel)
    bool derived;           // ... some of them derived (type remapping: k_derived_lines after those), or a value
                            // stage has a guard there (then also without URI stages)
    int n_uri, n_query;     // URI / query stages (the URI kernel instance)
    void* mid_event = nullptr;  // hipEvent_t recorded between the parse kernels and the URI kernels
    uint32_t chunk_lines = 0;   // lines per byte chunk the chunked kernel aims for (0: default)
    int32_t chunk_wait = 0;     // polls for a chunk's line number before deferring it (0: default, < 0: none)
    bool lit_aware = true;      // the program has a [^\s]* / "$request" element a shorter end of which can meet
                                // its literal (the chunked kernel's instance with literal-aware first candidates)
    bool simple = false;        // one format of the Apache common / combined family (capi simple_program)
    bool multi = false;         // several LogFormats (match words in the chunk kernel, then the routing scan)
    int shape = 0;              // the fixed shape whose chunk kernel instance parses the program (lp_fixed.h
                                // fixed_shape_of; FS_NONE: the instances per program class)
    bool geoip = false;         // the program has GeoIP value stages (k_geoip_lines after the URI kernels)
    void* geo_event[2] = {nullptr, nullptr};  // hipEvent_t recorded before / after k_geoip_lines
};
// The chunked parse kernel's geometry: cb input bytes per chunk (one wave
// each), an LDS window of win_cap bytes (the chunk, 64 bytes before it, the
// tail of its last line), n_chunks chunks.
struct ChunkPlan {
    uint32_t cb, win_cap, stk_words;  // stk_words: the DFS stack of the queued lines' kernels (the chunk kernels have none)
    int waves_per_cu;
    size_t lds;
    int64_t n_chunks;
};
ChunkPlan chunk_plan(const ParseLaunch& a);
// parse every line of a device program, then the URI stages (k_uri_lines, and
// its direct path), then meta->counters[0..4] += lines, ok, bad, fallback,
// arena bytes written.  k_parse_chunks writes the line index, meta->n_lines /
// cap_ovf and the lines' rows, k_parse_ovf_lines the lines it queued; with
// several LogFormats k_route_ovf and the routing scan run between the two
// (C.chunk_state zeroed, C.chunk_counts and C.deferred_chunks: chunk_plan().n_chunks records,
// C.ovf_lines: cap_lines + 1 entries, C.uri_ovf_list: parse_waves(cap_lines) + 1).
// C: the host copy of the columns the device holds.
int launch_parse(const ParseLaunch& a, const DeviceArgs* d_args, const Columns& C, hipStream_t s);
// k_parse_chunks of the fixed shape a.shape on `grid` blocks (parse_fixed.hip); -1: no such instance
int launch_chunks_fixed(const ParseLaunch& a, const DeviceArgs* d_args, const ChunkPlan& cp, unsigned grid,
                        hipStream_t s);
// the URI kernels of a launch (uri.hip)
int launch_uri(const ParseLaunch& a, const DeviceArgs* d_args, hipStream_t s);
// k_geoip_lines of a launch whose program has GeoIP value stages (geoip.hip)
int launch_geoip(const ParseLaunch& a, const DeviceArgs* d_args, hipStream_t s);
// meta->counters[0..5] += the sum of n_entries count records (per_group: of
// 64-line groups, only those holding the batch's meta->n_lines lines)
int launch_reduce_counts(const uint32_t* d_wave_counts, int64_t n_entries, bool per_group, Meta* d_meta, hipStream_t s);
#if defined(LP_PROFILE)
int prof_read_parse(unsigned long long* out);
int prof_clear_parse();
int prof_read_parse_fixed(unsigned long long* out);  // (the fixed-shape instances' own points, parse_fixed.hip)
int prof_clear_parse_fixed();
int prof_read_uri(unsigned long long* out);
int prof_clear_uri();
#endif
// the sticky routing scan: C.fmt_match (every line's match word, written by
// the parse kernels) -> C.fmt_id (C.fmt_chunk: fmt_chunks()+1 words, the
// state after the last line at [fmt_chunks(n_lines)])
constexpr int FMT_CHUNK = 4096;
__host__ __device__ inline int64_t fmt_chunks(int64_t n_lines) { return (n_lines + FMT_CHUNK - 1) / FMT_CHUNK; }
int launch_route(const DeviceArgs* d_args, int64_t cap_lines, hipStream_t s);

// run histograms of the parsed batch (buf: its input) into hist
// (HIST_WORDS u64, zeroed here): layout in include/logparser_amd.h
constexpr int HIST_WORDS = 1024;
int launch_histograms(const DeviceArgs* d_args, const uint8_t* buf, int64_t cap_lines, uint64_t* hist, hipStream_t s);

// device table (table.hip, lp_table.h): scratch bytes for count rows; the
// values / validity / STRING offsets of rows [ta.first, ta.first + ta.count)
// (d_targs: ta on the device; buf: the batch's input); then, once the caller
// checked the offsets' totals against its capacities, the STRING bytes
size_t table_scratch_bytes(int64_t count, int n_str);
// where TableArgs::srcw starts in that scratch
size_t table_srcw_offset(int64_t count);
// the table runs the kernels' row-list instances (a row list or a pseudo-column,
// lp_table.h): ta.bad_row is then zeroed by launch_table_values and read by the
// caller with the STRING totals
bool table_ext(const TableArgs& ta);
// mid (optional): recorded after k_table_values, before the offset scans;
// offsets false: no scans, a STRING column's i64[k + 1] stays row k's length
int launch_table_values(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const uint8_t* buf,
                        void* scratch, size_t scratch_bytes, hipStream_t s, hipEvent_t mid = nullptr, bool offsets = true);
int launch_table_chars(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const uint8_t* buf,
                       hipStream_t s);

// a map column of the device table (lp_table.h MapArgs), three launches with a
// read of totals between them: scratch bytes for count rows whose column has
// `pieces` pieces (0: not known yet -- the per-row part, which stays where it
// is when the scratch grows no further);
//   launch_map_count   valid, the piece counts and bases; *total: the device
//                      word that will hold the piece count
//   launch_map_entries (ma.n_pieces set, > 0) the surviving pieces, their
//                      lengths and the scans; totals[0..2]: the device words
//                      of the entry count (u32), key bytes and value bytes
//   launch_map_fill    (the totals fit the caller's buffers) offsets and bytes
// Each binds ma's scratch pointers itself.
// With ma.rows set (lp_result_table_map_rows) launch_map_count zeroes and binds
// ma.bad_row (a device word: a row index outside the batch), which the caller
// reads with the piece total.
size_t map_scratch_bytes(int64_t count, int64_t pieces);
int launch_map_count(const DeviceArgs* d_args, MapArgs& ma, void* scratch, size_t scratch_bytes, hipStream_t s,
                     const int64_t** total);
int launch_map_entries(const DeviceArgs* d_args, MapArgs& ma, const uint8_t* buf, void* scratch, size_t scratch_bytes,
                       hipStream_t s, const void* totals[3]);
int launch_map_fill(MapArgs& ma, int64_t n_entries, void* scratch, size_t scratch_bytes, hipStream_t s);

// a dictionary-encoded STRING column of the device table (dict.hip, lp_table.h
// DictArgs, lp_dict.h), one column at a time in one scratch.  DictLayout: the
// byte offsets of the column's scratch arrays for count rows.  `table` is the
// scratch launch_table_values gets for the dictionary's values; the slot
// table, dead by then, shares its bytes; `dump` (the validity bytes of the
// dictionary's rows, all 1) shares the slot words'.  Per row: 8 + 8 (table /
// slots, 2 count + 1 words) + 8 (len) + 8 (srcw) + 4 (slot) + 4 + 4 (flag, rank)
// + 8 (reps) = 44 bytes, plus the scans' temporaries.
//   launch_dict_insert  the table reset (every call), then one lane per valid
//                       row: hash, probe, claim or min
//   launch_dict_rank    the representatives' flags and their scan; *total: the
//                       device word that will hold the dictionary's length
//   launch_dict_index   index[k], and the representatives' lines (rows null:
//                       first + k) for the dictionary's values
struct DictLayout {
    size_t table, table_bytes, len, srcw, slot, flag, rank, reps, tmp, tmp_bytes, words, total;
    uint32_t cap;
};
DictLayout dict_layout(int64_t count);
// binds da's scratch pointers and ta's (one STRING column: i64 = len, srcw, bad_row)
void dict_bind(DictArgs& da, TableArgs& ta, const DictLayout& L, void* scratch);
int launch_dict_insert(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const DictArgs& da,
                       const uint8_t* buf, hipStream_t s);
int launch_dict_rank(const DictArgs& da, const DictLayout& L, void* scratch, hipStream_t s, const uint32_t** total);
int launch_dict_index(const TableArgs& ta, const DictArgs& da, hipStream_t s);

// lp_result_select on a device view (select.hip): the lines of [first, first +
// count) (count > 0) whose status is in mask, ascending, as int64 line indices.
// One lane takes 16 lines, one wave SEL_WAVE_LINES, one block SEL_BLOCK_LINES
// (counted from first rounded down to 16).
//   launch_select_count  the blocks' match counts and their scan; *total: the
//                        device word that will hold the number of matches
//   launch_select_write  (the total fits rows) the indices
// from_bits (lp_result_select_where): both passes take their match words from
// the scratch's bit words -- select_bits(), one per 64 lines counted from first
// rounded down to 16, which launch_where_eval filled (where.hip; lp_table.h
// WhereArgs) -- instead of from status and mask.
constexpr int SEL_WAVE_LINES = 1024;
constexpr int SEL_BLOCK_LINES = 4096;
size_t select_scratch_bytes(int64_t first, int64_t count);
uint64_t* select_bits(int64_t first, int64_t count, void* scratch, size_t scratch_bytes);  // null: the scratch is short
int launch_select_count(const uint8_t* status, int64_t first, int64_t count, uint32_t mask, void* scratch,
                        size_t scratch_bytes, hipStream_t s, const int64_t** total, bool from_bits = false);
int launch_select_write(const uint8_t* status, int64_t first, int64_t count, uint32_t mask, int64_t* rows, void* scratch,
                        size_t scratch_bytes, hipStream_t s, bool from_bits = false);
// k_where_eval: the predicate of wa over the lines [wa.first, wa.first + wa.count)
// (count > 0), term t's value the column ta.cols[t] (d_targs: ta on the device),
// one bit per line into wa.bits
int launch_where_eval(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const uint8_t* buf,
                      const WhereArgs& wa, hipStream_t s);

// lp_result_group on a device view (group.hip, lp_group.h): GroupArgs.  The rows are
// a TableArgs' (first / count or rows, n_lines, bad_row); its columns without
// output pointers are the n_keys keys (kind 1 STRING / 2 LONG), then the
// distinct measures (LONG).  Scratch: hash [count] each row's key hash, valid
// [count] 1 for a row inside the batch, and the dictionary's slots [cap] /
// slot / flag / rank / reps (lp_table.h DictArgs, bound to the same arrays:
// k_dict_mark, the rank scan and k_dict_index number the groups).  acc:
// n_groups x A.n_words accumulator words, group-major.
struct GroupArgs {
    int64_t count;
    int32_t n_keys, hash_bits;  // hash_bits: LP_OPT_DICT_HASH_BITS
    uint32_t cap;
    int32_t peel;               // the direct regime's peel rounds (0: none)
    LP_G uint64_t* hash;
    LP_G uint8_t* valid;
    LP_G uint32_t *slots, *slot;
    LP_G uint32_t* fail;        // set when a probe ran out
    const LP_G int32_t* group_of;
    LP_G int64_t* acc;
    int64_t n_groups;
    GroupAccs A;
};
// the caller's arrays of the aggregates (k_group_finish)
struct GroupOut {
    int64_t groups;  // min(n_groups, groups_cap)
    LP_G int64_t* value[GROUP_MAX_AGGS];
    LP_G uint8_t* valid[GROUP_MAX_AGGS];
};
// The call's launches (group.hip).
// GroupLayout: the byte offsets of the call's scratch arrays for count rows,
// beside DictLayout -- the slot table (2 count + 1 words: 8 bytes per row), hash
// 8, slot 4, flag 4, rank 4, reps 8, valid 1, group_of 4 (used when the caller
// passes none): 41 bytes per row, plus the rank scan's temporaries; d.tmp /
// d.tmp_bytes are what launch_dict_rank reads.  The accumulators are not part
// of it: their size is known only once the groups are counted.
//   launch_group_insert  the table reset, then one lane per row: the key
//                        tuple's hash, stored, and lp_dict.h's insert
//   (launch_dict_rank / launch_dict_index on the DictArgs group_bind fills:
//   the groups' first rows, their numbers, group_of and the representatives)
//   launch_group_agg     (ga.n_groups, ga.acc, ga.group_of set) the words'
//                        identities, then one lane per row: privatised in LDS
//                        when n_groups x words <= lds_words, else direct with
//                        ga.peel peel rounds; *privatised: which one ran
//   launch_group_finish  value / valid of go.groups groups out of the words
struct GroupLayout {
    size_t slots, hash, slot, flag, rank, reps, valid, group_of, words, total;
    DictLayout d;
    uint32_t cap;
};
GroupLayout group_layout(int64_t count);
// binds ga's and da's scratch pointers (da.index: the caller's group_of, or the scratch's) and ta.bad_row
void group_bind(GroupArgs& ga, DictArgs& da, TableArgs& ta, const GroupLayout& L, void* scratch, int32_t* group_of);
int launch_group_insert(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const GroupArgs& ga,
                        const uint8_t* buf, hipStream_t s);
int launch_group_agg(const DeviceArgs* d_args, const TableArgs* d_targs, const TableArgs& ta, const GroupArgs& ga,
                     const uint8_t* buf, int64_t lds_words, hipStream_t s, bool* privatised);
int launch_group_finish(const GroupArgs& ga, const GroupOut& go, hipStream_t s);

// The Arrow export's packaging on device memory (arrow.hip).
//   launch_arrow_validity  n_cols columns' valid bytes [n_rows] (n_rows > 0; any
//                          alignment) -> their validity bitmaps, each ((n_rows +
//                          7) / 8 rounded up to 64) bytes, all written, and the
//                          count of valid rows ADDED to *count (the caller zeroes
//                          it on the stream before).  One lane takes 16 rows, one
//                          wave ARROW_WAVE_ROWS, one block ARROW_BLOCK_ROWS.
//   launch_arrow_narrow32  out[k] = (int32) in[k], k < n (n > 0)
constexpr int ARROW_WAVE_ROWS = 1024;
constexpr int ARROW_BLOCK_ROWS = 4096;
constexpr int ARROW_MAX_COLS = 32;  // columns per launch (the argument table travels as the kernel's argument)
struct ArrowValidCol {
    const uint8_t* valid;
    uint8_t* bitmap;
    unsigned long long* count;
};
struct ArrowValidArgs {
    ArrowValidCol col[ARROW_MAX_COLS];
};
int launch_arrow_validity(const ArrowValidArgs& A, int n_cols, int64_t n_rows, hipStream_t s);
int launch_arrow_narrow32(const int64_t* in, int32_t* out, int64_t n, hipStream_t s);

}  // namespace lp
