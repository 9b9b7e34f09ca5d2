// Typed output columns built on the device (lp_result_table on a device
// view): for each requested "TYPE:path" the planner names the device column
// its value comes from (per LogFormat), and two kernels fill the caller's
// columns -- values and per-row string lengths, then (after a scan of the
// lengths) the string bytes -- in the Arrow layout of include/logparser_amd.h.
// The per-row choice mirrors Plan::replay exactly for the kinds below; a path
// the replay derives in any other way stays on the host table.
#pragma once
#include <stdint.h>

#include "lp_program.h"

namespace lp {

enum : int32_t {
    TC_NONE = 0,   // not delivered for this LogFormat
    TC_TOKEN,      // a = token slot: the value (null: "-")
    TC_CLF2NUM,    // a = token slot: ConvertCLFIntoNumber (null -> 0L, else the value)
    TC_NUM2CLF,    // a = token slot: ConvertNumberIntoCLF ("0" -> null, else the value)
    TC_TIME,       // a = time stage, b = TF_* field, c = 1: the _utc group
    TC_FL,         // a = first-line stage, b = 0 method / 1 uri / 2 protocol
    TC_PROTO,      // a = first-line stage, b = 0 protocol / 1 version (of its protocol)
    TC_URI,        // a = URI stage, b = UP_* part
    TC_QP,         // a = query stage, b / c = offset / length of the name in TableArgs::names (the last occurrence)
    TC_NULL,       // always null (HttpUriDissector's userinfo)
    TC_SECMS,      // a = SECOND_MILLIS stage: its milliseconds (b = 1: x 1000, MICROSECONDS)
    TC_LIST,       // a = upstream list stage, b = item, c = 0 value / 1 redirected
    TC_LIST_MS,    // a = SECOND_MILLIS list stage, b = item, c bit 0: redirected, bit 1: MICROSECONDS
    TC_BINIP,      // a = BinaryIP stage: its bytes as signed decimals joined by '.'
    TC_PAIR,       // a = pair stage (cookie / raw query), b / c = offset / length of the name in TableArgs::names (the last occurrence)
    TC_SETC,       // a = Set-Cookie pair stage | SC_* field << 8, b / c = the cookie name in TableArgs::names:
                   // ResponseSetCookieDissector on the name's last cookie string
    // the pseudo-columns ("@line" / "@offset" / "@lineno" / "@status"): what the record reader knows of a
    // line without dissecting it (ApacheHttpdLogfileRecordReader.java:246-287: the line's text, its
    // LongWritable key), valid for every row whatever its status; the same for every LogFormat
    TC_LINE,       // STRING: the line's bytes [line_off[i], line_off[i + 1] - 1) less the '\r' of "\r\n"
    TC_OFFSET,     // LONG: line_off[i]
    TC_LINENO,     // LONG: TableArgs::first_line + i
    TC_STATUS,     // LONG: status[i]
    // a re-dissected remapped value (lp_program.h ValStage; after the pseudo-columns: their numbers stay)
    TC_SCREEN,     // a = value stage, b = 0 width / 1 height: that part of split("x") (a sub-span of the value)
    TC_UNIQUEID,   // a = value stage, b = UQ_* field of the decoded mod_unique_id
    TC_GEOIP,      // a = value stage, b = GF_* field, c = GK_* kind: the field of the record geo[a][row] names,
                   // gathered from the stage's field table (lp_geoip.h)
};
constexpr bool tc_pseudo(int32_t kind) { return kind >= TC_LINE && kind <= TC_STATUS; }
// ResponseSetCookieDissector outputs (dissectors/ResponseSetCookieDissector.java:49-58)
enum : int32_t { SC_VALUE, SC_EXPIRES_S /* STRING:expires, seconds */, SC_EXPIRES_MS /* TIME.EPOCH:expires */,
                 SC_DOMAIN, SC_COMMENT, SC_PATH };
enum : int32_t { TF_EPOCH, TF_DAY, TF_MONTHNAME, TF_MONTH, TF_WEEK, TF_WEEKYEAR, TF_YEAR, TF_HOUR, TF_MINUTE,
                 TF_SECOND, TF_MILLI, TF_MICRO, TF_NANO, TF_DATE, TF_TIME };
// ModUniqueIdDissector outputs, in delivery order (dissectors/ModUniqueIdDissector.java:117-131)
enum : int32_t { UQ_EPOCH, UQ_IP, UQ_PROCESSID, UQ_COUNTER, UQ_THREADINDEX };
enum : int32_t { UP_QUERY, UP_PATH, UP_REF, UP_PROTOCOL, UP_HOST, UP_PORT };

struct TableSrc {
    int32_t kind, a, b, c;
};

constexpr int MAX_TABLE_COLS = 32;
constexpr int TABLE_NAMES = 2048;

struct TableCol {
    int32_t kind;  // LP_CAST_STRING 1 / LONG 2 / DOUBLE 4
    int32_t pad;
    TableSrc src[MAX_FMT];
    // an earlier delivery of the same path (TC_NONE: none): the row's value
    // when src delivers none (ParsedRecord: a null is ignored, the last value
    // wins) -- a token that a converter of another token delivers again
    TableSrc alt[MAX_FMT];
    LP_G uint8_t* valid;
    LP_G int64_t* i64;   // STRING: offsets [count + 1]; LONG: values
    LP_G double* f64;
    LP_G uint8_t* chars;
};

// a STRING column's value of one row as k_table_values found it, for
// k_table_chars (TableArgs::srcw): tag in bits 63:62 -- SW_PTR the bytes'
// address (bit 61: a leading '&'), SW_LONG a long in bits 61:0 (two's
// complement), SW_SLOW anything else (a formatted date / time / month name /
// binary IP, or a long outside 62 bits): k_table_chars derives it again
constexpr uint64_t SW_AMP = 1ull << 61, SW_LONG = 1ull << 62, SW_SLOW = 2ull << 62;

struct TableArgs {
    int64_t first, count;
    int32_t n_cols, pad;
    LP_G uint64_t* srcw;  // [STRING column rank][count] value words (scratch)
    // row k is line rows[k] (lp_result_table_rows; null: line first + k).  An
    // index outside [0, n_lines) is never dereferenced: the row is valid 0 and
    // *bad_row is set (zeroed before the launch).  Read by the kernels'
    // row-list instances only (table.hip), which also serve the pseudo-columns.
    const LP_G int64_t* rows;
    LP_G uint32_t* bad_row;
    int64_t n_lines, first_line;  // the batch's line count; lp_result.first_line (TC_LINENO)
    TableCol cols[MAX_TABLE_COLS];
    uint8_t names[TABLE_NAMES];
};

// ---- a map column (lp_result_table_map on a device view): the wildcard's
// members are the pieces of one query stage (q_count / q_params) or one pair
// stage (p_count / p_tab) per LogFormat
enum : int32_t { MS_NONE = 0, MS_QUERY, MS_PAIR };  // a = the stage
struct MapSrc {
    int32_t kind, a;
};

// One column's kernel arguments (passed by value).  Scratch arrays: per row
// [count + 1] cnt / pbase (piece counts, their exclusive scan: pbase[count] =
// n_pieces); per piece [n_pieces + 1] flag / eidx (survives, its exclusive
// scan: eidx[n_pieces] = the entries), klen / vlen (key / value bytes of a
// surviving piece, else 0) and kpos / vpos (their exclusive scans); ksrc /
// vsrc [n_pieces] where the bytes are (SW_PTR words), ksrc_e / vsrc_e the
// same per entry (they reuse klen / vlen, dead after the scans).
struct MapArgs {
    int64_t first, count, n_pieces;
    const LP_G int64_t* rows;  // row k is line rows[k] (lp_result_table_map_rows; null: line first + k)
    LP_G uint32_t* bad_row;    // set when a rows[k] is outside [0, n_lines) (such a row: valid 0, no pieces)
    int64_t n_lines;
    MapSrc src[MAX_FMT];
    LP_G uint8_t* valid;
    LP_G int64_t *entry_off, *key_off, *val_off;
    LP_G uint8_t *key_chars, *val_chars;
    LP_G int64_t *cnt, *pbase;
    LP_G uint32_t *flag, *eidx;
    LP_G int64_t *klen, *vlen, *kpos, *vpos;
    LP_G uint64_t *ksrc, *vsrc, *ksrc_e, *vsrc_e;
};

// ---- a dictionary-encoded STRING column (lp_result_table_dict on a device
// view, dict.hip).  Kernel arguments passed by value; the column itself is
// cols[0] of a one-column TableArgs, whose k_table_values run left each row's
// validity (valid), length (len[k + 1]) and source word (srcw[k]).  Scratch:
// slots [cap] the open-addressing table of row numbers (lp_dict.h), slot [count]
// the slot each valid row ended in, flag / rank [count] the representatives
// (a row whose slot holds the row itself) and their inclusive scan
// (rank[count - 1] = the dictionary's length), reps [count] the representatives'
// lines in ascending row order: the row list the dictionary's values are
// built from.
struct DictArgs {
    int64_t count;
    uint32_t cap;
    int32_t hash_bits;  // LP_OPT_DICT_HASH_BITS
    const LP_G uint8_t* valid;
    const LP_G int64_t* len;
    const LP_G uint64_t* srcw;
    LP_G uint32_t *slots, *slot, *flag, *rank;
    LP_G uint32_t* fail;  // set when a probe ran out
    LP_G int32_t* index;  // the caller's [count]
    LP_G int64_t* reps;
};

// ---- lp_result_select_where on a device view (where.hip): term t's value is
// column t of a TableArgs without output pointers (its src / alt per LogFormat,
// its kind 1 STRING / 2 LONG, the names pool; rows null, n_lines / first_line
// set); its rule travels here, by value.  A STRING operand is
// TableArgs::names[str_off, str_off + str_len), after the columns' names.
// bits: one word per 64 lines counted from first rounded down to 16 -- the
// lines of select.hip's 16-line groups -- bit b of word w set when line (first
// & ~15) + 64 w + b is selected; every word that holds a line of the window is
// written whole.
constexpr int WHERE_MAX_TERMS = 8;
struct WhereTerm {
    int32_t op, group;  // lp_pred.h PRED_* (| PRED_NEGATE); terms of one group are OR-ed, the groups AND-ed
    int32_t str_off, str_len;
    int64_t lo, hi;
};
struct WhereArgs {
    int64_t first, count;
    int32_t n_terms;
    uint32_t mask;  // the status mask
    LP_G uint64_t* bits;
    WhereTerm t[WHERE_MAX_TERMS];
};

}  // namespace lp
