/*
 * logparser_amd -- MI355X (gfx950) batch engine for logparser's per-line hot
 * path: match Apache HTTPD access-log lines against a LogFormat and extract
 * typed fields (tokens, epoch-millisecond timestamps, request first line,
 * URI parts, percent-decoded query parameters).
 *
 * Drop-in boundary.  Every entry point below replaces a piece of the
 * reference's per-line Java path (paths relative to the reference repo,
 * hp/ = httpdlog/httpdlog-parser/src/main/java/nl/basjes/parse/httpdlog/,
 * core/ = parser-core/src/main/java/nl/basjes/parse/core/):
 *
 *   lp_compile        new HttpdLoglineParser<>(cls, logformat) + addParseTarget(...)
 *                     + the lazy Parser.assembleDissectors on first parse
 *                     (hp/HttpdLoglineParser.java:44-50,104-126;
 *                      core/Parser.java:237-356, 581-635;
 *                      hp/dissectors/tokenformat/TokenFormatDissector.java:127-213)
 *   lp_possible_paths Parser.getPossiblePaths() (core/Parser.java:904-1012)
 *   lp_parse_batch    a loop of Parser.parse(record, line) over a batch of
 *                     '\n'-separated lines (core/Parser.java:716-756), i.e.
 *                     HttpdLogFormatDissector.dissect + TokenFormatDissector.dissect
 *                     (hp/HttpdLogFormatDissector.java:173-204,
 *                      hp/dissectors/tokenformat/TokenFormatDissector.java:243-275)
 *                     and the downstream TimeStamp / HttpFirstLine / HttpUri /
 *                     QueryStringField / CLF converter dissectors -- run on the GPU.
 *   lp_line_status    the per-line outcome the caller's loop sees
 *                     (ApacheHttpdLogfileRecordReader.java:256-269): OK, BAD
 *                     (= DissectionFailure), FALLBACK (= not proven on device:
 *                     hand the line to the reference Java dissector).
 *   lp_line_record_json  the values the reference would have delivered to the
 *                     record's setters for that line (Parser.store,
 *                     core/Parser.java:760-876), as a canonical JSON object.
 *   lp_counters       the RecordReader counters "Lines read / Good lines /
 *                     Bad lines" (ApacheHttpdLogfileRecordReader.java:118-120)
 *                     plus the FALLBACK count.
 *   lp_result_*       the whole batch's SoA results in bulk: what a Java
 *                     GpuHttpdLogFormatDissector replays into
 *                     Parsable.addDissection (core/Dissector.java:62-186,
 *                     core/Parsable.java:77-140), see INTEGRATION.md.
 *
 * Threading: like the reference Parser (not thread-safe), one handle per
 * host thread / GPU.  Ownership: the caller owns the input buffer; the
 * handle owns device scratch and results until the next lp_parse_batch or
 * lp_free.  No torch types cross this boundary.
 */
#ifndef LOGPARSER_AMD_H
#define LOGPARSER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes */
#define LP_OK 0
#define LP_E_INVALID (-1)      /* bad arguments / logformat (InvalidDissectorException) */
#define LP_E_MISSING (-2)      /* MissingDissectorsException */
#define LP_E_UNSUPPORTED (-3)  /* compiled, but some requested path needs a dissector
                                  not implemented on the device: every line -> FALLBACK */
#define LP_E_DEVICE (-4)       /* HIP error / no device / extension not usable */
#define LP_E_NOMEM (-5)
#define LP_E_STATE (-6)        /* called in the wrong order */

/* per-line status */
#define LP_LINE_OK 0
#define LP_LINE_BAD 1          /* the reference throws DissectionFailure */
#define LP_LINE_FALLBACK 2     /* outside the device's proven subset */

/* lp_parse_batch buffer flags */
#define LP_BUF_HOST 0          /* host memory: copied H2D on the stream */
#define LP_BUF_DEVICE 1        /* device pointer, already resident in HBM */

typedef struct lp_handle lp_handle;

/* Compile a LogFormat (one or more, '\n' separated; aliases common /
 * combined / combinedio / referer / agent) and the requested "TYPE:path"
 * targets.  device: HIP device ordinal.  Returns NULL on failure; *status
 * receives LP_OK / LP_E_UNSUPPORTED (handle still usable) / error code. */
lp_handle *lp_compile(const char *logformats, const char *const *paths, int n_paths,
                      int device, int *status, char *err, size_t errlen);

/* Parser.addTypeRemapping(input, newType, casts) (core/Parser.java:636-677):
 * a value delivered at path `input` is delivered again as type `type`
 * (Parsable.addDissection, core/Parsable.java:160-176), where that type's
 * dissectors take it further (Parser.java:446-455): e.g. a query parameter
 * holding a URL, remapped to HTTP.URI, is dissected by HttpUriDissector on
 * the device (the "derived" URI stages).  casts: LP_CAST_* bits of the
 * remapped target (the reference's STRING_ONLY default is LP_CAST_STRING). */
typedef struct lp_remap {
    const char *input;
    const char *type;
    int32_t casts;
} lp_remap;
/* lp_compile with the parser's type remappings (n_remaps may be 0). */
lp_handle *lp_compile_remapped(const char *logformats, const char *const *paths, int n_paths,
                               const lp_remap *remaps, int n_remaps, int device, int *status, char *err,
                               size_t errlen);

/* Parser.addDissector(dissector) (core/Parser.java:154-160): a dissector of
 * the reference's httpdlog-parser jar that is not registered by default, by
 * class name as Hive's "load:" / Pig's "-load:" give it, with their settings
 * string.  Known: "ScreenResolutionDissector" (also
 * "nl.basjes.parse.httpdlog.dissectors.ScreenResolutionDissector"): a value
 * remapped to SCREENRESOLUTION delivers SCREENWIDTH:<path>.width and
 * SCREENHEIGHT:<path>.height.  The settings are accepted and kept, but the
 * value is split on "x" whatever they say: the reference dissects with a
 * fresh instance that never sees them.  Registering a class twice is the same
 * as once; any other name is LP_E_INVALID.  settings may be NULL ("").
 *
 * The GeoIP classes "GeoIPCountryDissector", "GeoIPCityDissector",
 * "GeoIPASNDissector" and "GeoIPISPDissector" (also
 * "nl.basjes.parse.httpdlog.dissectors.geoip.<Class>"): settings is the path
 * of a MaxMind DB file, read when the handle is compiled.  Below every
 * IP-typed path (%h, %a, %A, $remote_addr, ..., or a token remapped to IP)
 * they deliver STRING:<p>.continent.name / .continent.code / .country.name /
 * .country.iso, NUMBER:<p>.country.getconfidence,
 * BOOLEAN:<p>.country.isineuropeanunion (Country); those and
 * STRING:<p>.subdivision.name / .subdivision.iso / .city.name / .postal.code /
 * .location.timezone, NUMBER:<p>.city.confidence / .city.geonameid /
 * .postal.confidence / .location.accuracyradius / .location.averageincome /
 * .location.metrocode / .location.populationdensity, and
 * STRING:<p>.location.latitude / .location.longitude (STRING | DOUBLE: the
 * value as Double.toString prints it) (City); ASN:<p>.asn.number and
 * STRING:<p>.asn.organization (ASN); those and STRING:<p>.isp.name /
 * .isp.organization (ISP).
 *   LP_E_INVALID      the file cannot be opened or is no valid database (err
 *                     names the class and the file), also for "" -- from
 *                     lp_compile_dissectors and lp_possible_paths_dissectors
 *   LP_E_UNSUPPORTED  (a handle whose every line is FALLBACK, the reason in
 *                     err) a class registered twice with different paths
 *                     (the same path twice counts as once); a database whose
 *                     database_type lacks the class's word (Country, City,
 *                     ASN, ISP); a requested path that two registered classes
 *                     deliver from one input (City and Country, ISP and ASN);
 *                     a source that is no captured token (a query parameter,
 *                     a cookie, a list item, $binary_remote_addr's value, a
 *                     mod_unique_id's .ip); more than 8 value stages
 * A line is LP_LINE_FALLBACK when a looked-up value is anything but a dotted
 * quad (four decimal parts 0-255, no leading zero) or RFC 4291 text (also
 * with a dotted quad as its last two groups) of at most 45 bytes -- a host
 * name would be resolved over DNS by the reference -- or an IPv6 address
 * against an ip_version 4 database.  "-", an empty value and an address that
 * is not in the database deliver nothing; an IPv4-mapped address
 * (::ffff:a.b.c.d) is looked up as IPv4. */
typedef struct lp_dissector {
    const char *name;
    const char *settings;
} lp_dissector;
/* lp_compile_remapped with registered dissectors (n_dissectors may be 0: the
 * same call).  Remapped values that are re-dissected on the device -- a
 * SCREENRESOLUTION (registered) or a MOD_UNIQUE_ID (ModUniqueIdDissector,
 * registered by default) -- must be a captured token or a requested query
 * parameter, at most 8 of them per program; a parameter that occurs twice on
 * a line, and a SCREENRESOLUTION whose split lacks a requested part (the
 * reference throws), make the line LP_LINE_FALLBACK. */
lp_handle *lp_compile_dissectors(const char *logformats, const char *const *paths, int n_paths,
                                 const lp_remap *remaps, int n_remaps, const lp_dissector *dissectors,
                                 int n_dissectors, int device, int *status, char *err, size_t errlen);
void lp_free(lp_handle *h);

/* Parser.getPossiblePaths(max_depth) for a logformat: '\n'-separated, sorted.
 * Returns the number of bytes written (excluding NUL) or a negative error. */
int64_t lp_possible_paths(const char *logformats, int max_depth, char *out, size_t cap);
/* The same with type remappings: each remapped path and what the new type's
 * dissectors produce below it (core/Parser.java:954-962). */
int64_t lp_possible_paths_remapped(const char *logformats, int max_depth, const lp_remap *remaps, int n_remaps,
                                   char *out, size_t cap);
/* The same with registered dissectors: a path remapped to SCREENRESOLUTION
 * lists its .width / .height below it, every IP-typed path the outputs of the
 * registered GeoIP classes.  LP_E_INVALID for an unknown class or a GeoIP
 * database that cannot be read. */
int64_t lp_possible_paths_dissectors(const char *logformats, int max_depth, const lp_remap *remaps, int n_remaps,
                                     const lp_dissector *dissectors, int n_dissectors, char *out, size_t cap);

/* Options (lp_set_option). */
#define LP_OPT_FORCE_DIRECT 1  /* 1: every wave reads its lines from HBM (no LDS window);
                                  diagnostics and tests of the direct path only */
#define LP_OPT_MAX_RETRIES 2   /* re-runs of a batch whose ARENA estimate was short (default 3,
                                  0..16); an arena still short after them degrades: the lines
                                  that did not fit are FALLBACK, lp_counters out[6].  A short
                                  line capacity is always re-run with the exact count (at most
                                  twice, not bounded by this option): nothing is parsed without
                                  columns for every line */
#define LP_OPT_ARENA_BYTES 3   /* tests: exact arena capacity of each batch's first run (0 = estimate) */
#define LP_OPT_CHUNK_LINES 4   /* one-format programs: lines per byte chunk the one-pass parse kernel
                                  aims for (1..64, 0 = default 54; a chunk's 65th line onwards is
                                  parsed from HBM by a second kernel) */
#define LP_OPT_CHUNK_WAIT 5    /* tests: polls a chunk's wave makes for its first line number before it
                                  leaves the chunk to the deferred pass (0 = default 16384; -1: none,
                                  every chunk goes to the deferred pass; -2: the odd chunks go to it
                                  without polling, the even ones wait as by default) */
#define LP_OPT_ONE_PASS 6      /* reserved: every device program is parsed in one pass over the input
                                  (several LogFormats: the chunk kernel routes every line exactly one
                                  format matches; the rest after the routing scan).  1 is accepted and
                                  changes nothing; 0, which once chose separate line index, routing
                                  and parse passes, is LP_E_INVALID */
#define LP_OPT_FIXED_SHAPE 7   /* 1 (default): a handle whose compiled program equals one of the fixed
                                  shapes (common, combined with every path requested) is parsed by
                                  that shape's instance of the chunk kernel, lp_counters out[11]
                                  (out[12]: lines of the batch whose first leaf that instance
                                  matched with the element walk, not the straight-line one);
                                  0: by the instances per program class, as every other program */
#define LP_OPT_DICT_HASH_BITS 8 /* tests: lp_result_table_dict on a device view keeps only this many low
                                  bits of a value's hash for its home slot (1..32; 0 = default, all 64
                                  bits): distinct values then collide, and a few hundred rows run the
                                  probe and byte-compare paths.  The result does not depend on it.
                                  lp_result_group on a device view narrows its key hash the same way,
                                  the home slot and the hash it stores per row: distinct key tuples
                                  then meet in the probe and in the full compare */
#define LP_OPT_GROUP_LDS_WORDS 9 /* tests, measurements: lp_result_group on a device view accumulates in
                                  per-block LDS copies when groups x accumulator words per group is at
                                  most this many 8-byte words, else with global atomics (1..8192; 0 =
                                  default 4096; -1: never in LDS).  The result does not depend on it */
#define LP_OPT_GROUP_PEEL 10   /* measurements: rounds in which a wave of lp_result_group's global-
                                  atomic regime merges the rows of its leading group into one atomic
                                  (1..4; 0 = default 2; -1: none).  The result does not depend on it */
int lp_set_option(lp_handle *h, int option, int64_t value);

/* Capacity for the coming batches: columns for max_lines lines and at least
 * arena_bytes of side arena (0 = estimated; the estimate wins when larger).
 * With it (or after a first batch, whose line count sizes the buffers)
 * lp_parse_batch enqueues the whole batch without waiting for the device; a
 * batch that outgrows the buffers is re-run with exact sizes inside lp_sync
 * (a short arena at most LP_OPT_MAX_RETRIES times, after which the lines that
 * did not fit go to FALLBACK instead of failing the batch; a short line
 * capacity at most twice, with the exact count). */
int lp_reserve(lp_handle *h, int64_t max_lines, uint64_t arena_bytes);

/* Parse every line of buf[0, nbytes), Hadoop LineRecordReader semantics
 * (ApacheHttpdLogfileRecordReader.java:57, 115): a line ends at '\n', at a
 * lone '\r' or at "\r\n", the terminator is not part of it, and a final
 * line without one counts.  stream: a hipStream_t (NULL = default stream).
 * Enqueues all work on the stream and returns without synchronizing (except a
 * handle's first batch without a reservation, which waits for its line
 * count); call lp_sync before reading results.  A batch still pending on the
 * handle is finished first: to overlap batches, use one handle per stream.
 * On error the handle holds no batch (the accessors return LP_E_STATE) until
 * a batch succeeds.
 * first_line_no (lp_parse_batch_at): the global number of the batch's first
 * line (a split reader's position in the stream); it comes
 * back in lp_result.first_line.  lp_parse_batch continues the handle's
 * numbering (0 for its first batch, then the previous batch's first line +
 * its line count). */
int lp_parse_batch(lp_handle *h, const uint8_t *buf, uint64_t nbytes, int buf_flags, void *stream);
int lp_parse_batch_at(lp_handle *h, const uint8_t *buf, uint64_t nbytes, int64_t first_line_no, int buf_flags,
                      void *stream);
int lp_sync(lp_handle *h);

/* Results of the last batch (after lp_sync). */
int64_t lp_num_lines(lp_handle *h);
/* copies statuses of lines [first, first+count) to host memory */
int lp_line_status(lp_handle *h, int64_t first, int64_t count, uint8_t *out);
/* byte offset of line i in the batch (i <= num_lines) */
int64_t lp_line_offset(lp_handle *h, int64_t i);
/* canonical record of line i (status must be OK):
 *   {"TYPE:path": [v, ...], ...}  keys sorted; v = "str" | null | {"l": n}
 * returns bytes written (excluding NUL) or negative (LP_E_STATE if the line
 * is not OK, -100 - needed if cap is too small). */
int64_t lp_line_record_json(lp_handle *h, int64_t i, char *out, size_t cap);
/* out[0..3] = lines, ok, bad, fallback of the last batch (device counters);
 * diagnostics: out[4] = lines the chunk kernel queued for the direct kernel,
 * which reads them from HBM (a byte chunk's 65th line onwards, a line ending
 * past the chunk's LDS window, and the lines out[9] counts; 0 when the
 * program is not on the device), out[5] = re-runs of the
 * batch (capacity / arena estimates exceeded), out[6] = arena overflows the
 * final run left (lines sent to FALLBACK for want of arena; 0 normally),
 * out[7] = waves whose URI bytes exceeded the URI kernel's compact buffer
 * (their URI stages read the input from HBM directly), out[8] = one-format
 * programs: byte chunks redone by the deferred pass (their wave stopped
 * waiting for its first line number; 0 normally, see LP_OPT_CHUNK_WAIT),
 * out[9] = lines the chunk kernel queued for the overflow kernels because
 * the first leaf of the match did not decide them (they need the backtracking
 * DFS, or the routing of a several-format program does); lines queued
 * because their chunk's window does not hold them, or as a chunk's 65th line
 * onwards, are not counted; out[10] = lines whose URI stages were redone
 * with the repair on (a malformed URI that HttpUriDissector repairs before
 * URI.create: bad '%' escapes, "&amp;" and numeric entities, "=#", "#&",
 * several '#'), out[11] = the fixed shape whose instance of the chunk kernel
 * parsed the batch (1 combined, 2 common; 0: none, see LP_OPT_FIXED_SHAPE).
 * Returns the words written (at most 12). */
int lp_counters(lp_handle *h, uint64_t *out, int n);

/* Device-side timing of the last batch, in milliseconds, measured with HIP
 * events on the batch's stream: [0] whole batch, [1] separate line index
 * kernels (a program that is not on the device; a device program's parse
 * kernel finds the lines itself: only the line count of a prefix, on a
 * handle's first batch without a reservation), [2] parse pass (every kernel
 * after the index), [3] of it the parse kernels (k_parse_chunks and
 * k_parse_ovf_lines; several LogFormats: k_route_ovf and the routing scan
 * between them), [4] of it the URI kernels (+ the counter reduction); then the last
 * complete lp_result_table on a device view: [5] k_table_values, [6] the
 * STRING columns' offset scans, [7] k_table_chars; then the last complete
 * lp_result_table_map on a device view, summed over its columns: [8]
 * k_map_count and the piece-base scan, [9] k_map_entries and its scans, [10]
 * k_map_fill and k_map_chars; then [11] the last complete lp_result_select on
 * a device view: k_select_count, the block scan, the host's read of the count
 * and k_select_write; then the last complete lp_result_table_dict on a device
 * view, summed over its columns: [12] k_table_values of the rows, [13] the
 * table reset and k_dict_insert, [14] k_dict_mark, the rank scan and
 * k_dict_index, [15] the dictionary's values (k_table_values, the offset scan
 * and k_table_chars over the representatives); then [16] the last complete
 * lp_result_arrow on a device view: its packaging kernels (k_arrow_validity's
 * bitmaps and counts, k_arrow_narrow32), summed over the columns.  [16] is
 * written only for n >= 17: a caller that passes 16 sees what it always saw;
 * [17], for n >= 18, is k_geoip_lines of the last batch (0 for a program
 * without a GeoIP stage; it is part of [4]); then the last complete
 * lp_result_select_where with terms on a device view: [18] k_where_eval, [19]
 * its compaction (k_select_count, the block scan, the host's read of the
 * count and k_select_write over the predicate's bits).  [18] and [19] are
 * written only for n >= 20: a caller that passes 18 sees what it always saw;
 * then the last complete lp_result_group on a device view: [20] the resets and
 * k_group_insert (the keys' values, their hash, the insert), [21] k_dict_mark,
 * the rank scan and k_dict_index (the groups' numbers), [22] the accumulators'
 * fill, k_group_agg and k_group_finish.  [20..22] are written only for n >= 23.
 * Returns the number of values written (at most 23). */
int lp_last_timing(lp_handle *h, float *out_ms, int n);

/* Run histograms of the last batch, computed on the device (SURVEY.md §5
 * counters; multi-GPU callers all-reduce them, e.g. over RCCL).  out: 1024
 * u64 words, host memory, or device memory on the handle's device when
 * out_on_device (then usable directly as an all-reduce buffer).  The batch's
 * input must still be valid.  Layout (word: count):
 *   0 lines, 1 OK, 2 BAD, 3 FALLBACK lines
 *   16 + k: OK lines whose captured token slot k is "-" (null)
 *   32 + k: OK lines whose token slot k is present and non-empty
 *   48: OK lines whose status value (token request.status.last, else
 *       request.status, if requested) is not a code 100..599
 *   64 + m: OK lines by request method (first-line dissector, if requested):
 *       m = 0 GET 1 POST 2 HEAD 3 PUT 4 DELETE 5 OPTIONS 6 PATCH 7 CONNECT
 *       8 TRACE 9 PROPFIND 10 MKCOL 11 COPY 12 MOVE 13 LOCK 14 UNLOCK
 *       15 other, 16 no method
 *   100 + c: OK lines with status code c (100 <= c <= 599)
 * Replaces the reference's Hadoop counters (ApacheHttpdLogfileRecordReader.java:118-120)
 * for a batch; returns LP_OK or an error. */
#define LP_HIST_WORDS 1024
#define LP_HIST_LINES 0
#define LP_HIST_OK 1
#define LP_HIST_BAD 2
#define LP_HIST_FALLBACK 3
#define LP_HIST_TOK_NULL 16
#define LP_HIST_TOK_PRESENT 32
#define LP_HIST_STATUS_OTHER 48
#define LP_HIST_METHOD 64
#define LP_HIST_STATUS 100
int lp_histograms(lp_handle *h, uint64_t *out, int out_on_device);

/* Algorithmic bytes of the last batch: [0] input bytes read, [1] bytes of
 * SoA results + arena written, [2] the parse kernels' bytes (input once,
 * line index, their columns), [3] the URI kernels' bytes (URI source bytes
 * gathered, the per-line columns they read, their columns and arena
 * writes) -- roofline accounting per kernel (timings [3] and [4]). */
int lp_last_bytes(lp_handle *h, uint64_t *out, int n);

/* ---- Bulk results: the SoA the kernels wrote (SURVEY.md §8(b) lp_result). ----
 * Per line i: status[i] (LP_LINE_*), and for the compiled program's stages
 * the columns listed in lp_result.column (name, stage index, element size,
 * byte offset from lp_result.columns), each n_lines elements:
 *   status (u8), tok_span[k] (u32 start | end << 16, line-relative) and
 *   tok_flags (u32: bit k value "-" = null, bit 16+k value "0") per captured
 *   token k; t_epoch[t] (i64 epoch ms), t_local[t] / t_utc[t] (u64 packed
 *   calendar, lp_program.h pack_cal), t_nano[t] (u32) per timestamp stage;
 *   fl_kind / fl_method / fl_uri / fl_proto (u32 kind, spans) per first-line
 *   stage; u_flags (u32 UF_* bits), u_scheme / u_host / u_path / u_query /
 *   u_frag (u64 refs) and u_port (i32) per URI stage; q_count (u32) and
 *   q_params (u64 ref of a table of q_count (name ref, value ref) pairs) per
 *   query stage; arena_base (u64, the line's arena region); fmt_id (u8, the
 *   routed LogFormat) with several LogFormats; geo[k] (u32) per GeoIP value
 *   stage k: the id + 1 of the database record the line's address led to, 0
 *   when nothing is delivered (the ids are the engine's own, dense per database).
 * A ref is off | len << 32 (len 30 bits); bit 63 set: the bytes are in the
 * line's arena region, else line-relative; bit 62: '&' followed by those
 * bytes.  A q_params table slot whose parameter name was not requested holds
 * ~0 (REF_SKIP) as its name ref: skip it.  Arena offsets b live in shard
 * s = b / shard_cap, at arena + shard_off[s] + (b - s * shard_cap). */
#define LP_ARENA_SHARDS 64
typedef struct lp_column {
    char name[16];
    int32_t index;
    int32_t elem_size;
    uint64_t offset;
} lp_column;
typedef struct lp_result {
    int64_t n_lines;
    int64_t first_line;        /* global number of line 0 of the batch (lp_parse_batch_at) */
    uint64_t input_bytes;
    const uint8_t *input;      /* line i = input[line_off[i], line_off[i+1] - 1), less the '\r' of a
                                  "\r\n" terminator; NULL if not copied */
    const uint64_t *line_off;  /* n_lines + 1 entries */
    const uint8_t *columns;
    uint64_t columns_bytes;
    const uint8_t *arena;
    uint64_t arena_bytes;
    uint64_t shard_cap;
    uint64_t shard_off[LP_ARENA_SHARDS];
    int32_t n_columns;
    int32_t on_host;           /* 0: device pointers (lp_result_view), 1: host copy (lp_result_copy) */
    const lp_column *column;   /* view: owned by the handle, valid until its next batch;
                                  host copy: inside the copy's buffer */
} lp_result;
/* Device pointers of the last batch's results (valid until the next batch). */
int lp_result_view(lp_handle *h, lp_result *out);
/* Copy the last batch's results (line index, columns, used arena, and the
 * input when with_input) into host memory (pinned memory copies fastest) in
 * one call.  Returns the bytes used, or -(bytes needed) when host is NULL or
 * cap is too small. */
int64_t lp_result_copy(lp_handle *h, void *host, uint64_t cap, int with_input, lp_result *out);
/* The canonical record of line i (as lp_line_record_json) from a host copy
 * made with the input: no device access. */
int64_t lp_result_record_json(lp_handle *h, const lp_result *r, int64_t i, char *out, size_t cap);

/* The reference's Parsable.addDissection(base, type, name, value) calls
 * that deliver line i's requested values (core/Parsable.java:77-193), from a
 * host copy made with the input, in the reference's emission order: what a
 * Java GpuHttpdLogFormatDissector.dissect replays.  kind:
 * LP_VALUE_STRING (bytes p[0, len), UTF-8), LP_VALUE_NULL, LP_VALUE_LONG (l).
 * Returns the number of calls, or LP_E_STATE when line i is not OK. */
#define LP_VALUE_STRING 0
#define LP_VALUE_NULL 1
#define LP_VALUE_LONG 2
typedef void (*lp_emit_fn)(void *ctx, const char *base, const char *type, const char *name, int kind,
                           const uint8_t *p, uint32_t len, int64_t l);
int lp_result_emit(lp_handle *h, const lp_result *r, int64_t i, lp_emit_fn fn, void *ctx);

/* Parser.getCasts(name) (parser-core/.../core/Parser.java:127-129, filled
 * at :438-439 from each dissector's prepareForDissect): the casts of a
 * "TYPE:path" the handle delivers, as LP_CAST_* bits (0 = NO_CASTS), or
 * LP_E_MISSING when no dissector delivers it.  The caller's setter side
 * (Parser.store, :760-876) needs them to pick String / Long / Double setters. */
#define LP_CAST_STRING 1
#define LP_CAST_LONG 2
#define LP_CAST_DOUBLE 4
int lp_casts(lp_handle *h, const char *target);

/* Typed columns of a batch, the output side of a parse: what a caller with
 * one setter per column type builds per line -- the Hadoop ParsedRecord
 * (httpdlog-inputformat/.../ParsedRecord.java:154-214: set(name, String /
 * Long / Double), nulls ignored, the last value wins) read back column by
 * column as the Hive SerDe does (httpdlog-serde/.../ApacheHttpdlogDeserializer.java:
 * 224-240 STRING / BIGINT / DOUBLE columns, :295-323 one row per line).
 * From a host copy (lp_result_copy with the input), rows [first, first+count):
 *   kind LP_CAST_STRING: i64 = byte offsets [count + 1] into chars (Arrow
 *        layout: row k = chars[i64[k], i64[k + 1])), chars_cap bytes at chars;
 *   kind LP_CAST_LONG:   i64 = values [count];  LP_CAST_DOUBLE: f64 = values;
 *   valid[k] = 1 when row k has a value (lines not OK have none).
 * path: a requested "TYPE:path" (a wildcard request's member by its full
 * path).  Returns LP_OK; LP_E_NOMEM when a STRING column's chars_cap is too
 * small (chars_len = bytes needed: call again); LP_E_MISSING for a path the
 * handle does not deliver; LP_E_INVALID when the path's casts (lp_casts) do
 * not include the column's type (the reference's store would call no setter).
 * threads: host threads to replay with.
 * On a device view (r from lp_result_view, on_host 0) the table is built on
 * the GPU from the batch still in HBM (its input must still be valid):
 * valid / i64 / f64 / chars are then device buffers of the handle's device,
 * the call returns once they are filled.  Request cookies, raw-token query
 * strings, Set-Cookie cookies and their value / expires / domain / comment /
 * path attributes, upstream list items (N.value / N.redirected, SECOND_MILLIS
 * in ms and us), BinaryIP, the first line / URI / query values, and the
 * outputs of the dissectors on a remapped token or query parameter
 * (SCREENWIDTH:<p>.width / SCREENHEIGHT:<p>.height of a SCREENRESOLUTION;
 * TIME.EPOCH:<p>.epoch, IP:<p>.ip, PROCESSID:<p>.processid, COUNTER:<p>.counter,
 * THREAD_INDEX:<p>.threadindex of a MOD_UNIQUE_ID) and the GeoIP classes'
 * outputs (STRING and LONG columns; location.latitude / .longitude also as
 * DOUBLE columns) are device columns.
 * LP_E_UNSUPPORTED names a path whose value only the host replay
 * derives (a converter applied to an already converted value) or a DOUBLE
 * column of a string-valued path (Double.parseDouble): build those from a
 * host copy. */
typedef struct lp_table_col {
    const char *path;
    int32_t kind;
    uint8_t *valid;
    int64_t *i64;
    double *f64;
    char *chars;
    uint64_t chars_cap;
    uint64_t chars_len;
} lp_table_col;
int lp_result_table(lp_handle *h, const lp_result *r, int64_t first, int64_t count, lp_table_col *cols, int n_cols,
                    int threads);

/* Wildcard targets of a batch as map columns: for a requested "TYPE:prefix.*"
 * (STRING:request.firstline.uri.query.*, HTTP.COOKIE:request.cookies.*,
 * STRING:request.querystring.*, HTTP.SETCOOKIE:response.cookies.*, ...) one
 * map<string,string> per row -- what the Hadoop record reader registers for a
 * ".*" field (httpdlog-inputformat/.../ApacheHttpdLogfileRecordReader.java:
 * 206-208: ParsedRecord.setMultiValueString), the record collects per line
 * (ParsedRecord.java:178-196: the key is the name after the prefix, a null
 * value is ignored, a later value of a key replaces the earlier; :210-212
 * getStringSet) and the Pig Loader returns as a DataType.MAP column
 * (httpdlog-pigloader/.../Loader.java:227-229, 389-390).  Members are the
 * values Parsable.addDissection delivers to the wildcard (lp_result_emit's
 * rule: the wildcard of the value's base and type); a member with an empty
 * name has the key "".  Java's HashMap has no order; here a surviving entry
 * stands at the position of its key's last non-null delivery, in delivery
 * order, the same from a host copy and on the device.
 * Rows [first, first+count), Arrow MapArray layout:
 *   valid[k] = 1 when line first+k is OK (its record exists; the map may be
 *        empty, as for every row of a LogFormat that does not deliver the
 *        path), 0 for a BAD or FALLBACK line (no entries);
 *   entry_off[count + 1]: row k's entries are [entry_off[k], entry_off[k + 1]);
 *   key_off / val_off [entries + 1] into key_chars / val_chars: entry e is
 *        key_chars[key_off[e], key_off[e + 1]) -> val_chars[val_off[e],
 *        val_off[e + 1]) (UTF-8; no value validity: a null never enters).
 * Sizes as lp_result_table: entries_cap (key_off and val_off hold
 * entries_cap + 1 words, never NULL), key_chars_cap, val_chars_cap; every call
 * sets entries_len / key_chars_len / val_chars_len to what the rows need.
 * Returns LP_OK; LP_E_NOMEM when a capacity is too small (all three lengths
 * set, the arrays' contents undefined: call again); LP_E_MISSING for a path
 * the handle does not deliver; LP_E_INVALID for a path that is not a wildcard.
 * threads: host threads to replay with.
 * On a device view (on_host 0) the columns are built on the GPU from the
 * piece tables the URI kernels wrote, and every array is a device buffer of
 * the handle's device.  LP_E_UNSUPPORTED there when something other than one
 * query-string stage or one cookie / raw query string / Set-Cookie stage per
 * LogFormat delivers under the prefix (a type remapping below it, two stages
 * under one name, a dissector's named outputs): build those from a host copy.
 * lp_last_timing [8..10]: the last device call's phases (piece counts; the
 * surviving pieces and their scans; offsets and bytes), summed over columns. */
typedef struct lp_table_map_col {
    const char *path;
    uint8_t *valid;
    int64_t *entry_off;
    int64_t *key_off;
    int64_t *val_off;
    char *key_chars;
    char *val_chars;
    uint64_t entries_cap;
    uint64_t key_chars_cap;
    uint64_t val_chars_cap;
    uint64_t entries_len;
    uint64_t key_chars_len;
    uint64_t val_chars_len;
} lp_table_map_col;
int lp_result_table_map(lp_handle *h, const lp_result *r, int64_t first, int64_t count, lp_table_map_col *cols,
                        int n_cols, int threads);

/* ---- Row selection: dense tables of chosen lines. ----
 * The reference's consumers never see a row for a line that did not parse:
 * the Hadoop record reader loops past a line that throws DissectionFailure
 * ("Ignore bad lines and simply continue") and returns the next good record,
 * keyed by the line's byte offset (httpdlog-inputformat/.../
 * ApacheHttpdLogfileRecordReader.java:246-277 nextKeyValue, :283-287
 * getCurrentKey); the Hive SerDe returns null for it (httpdlog-serde/.../
 * ApacheHttpdlogDeserializer.java:284-291); the Pig loader reads through the
 * same record reader.  lp_result_select names the lines of a window whose
 * status is in a mask; the *_rows calls build the typed table / the map
 * columns of exactly those lines; the pseudo-columns carry the line's text
 * and keys.  Together: the dense table of the OK lines (LP_SEL_OK), the few
 * lines the host parser must redo with their text (LP_SEL_FALLBACK, "@line")
 * and the key to merge both results ("@lineno" / "@offset").
 *
 * lp_result_select: the lines of [first, first+count) whose status is in
 * status_mask (LP_SEL_* bits), ascending, as batch-relative line indices (NOT
 * window-relative).  The table's size protocol: *rows_len is always set to the
 * number of selected lines; LP_E_NOMEM when rows_cap is smaller (nothing is
 * written then: call again), else LP_OK with rows[0, *rows_len) filled.
 * Mask 0 selects nothing; a bit other than the three gives LP_E_INVALID.  On
 * a device view (on_host 0) rows is a device buffer of the handle's device and
 * the selection is a stream compaction on the GPU (one host read of the count
 * between its two passes); on a host copy rows is host memory.  State and
 * window checks as lp_result_table.  lp_counters out[1..3] already are the
 * exact sizes of a whole-batch select of one status: one call suffices there.
 * lp_last_timing [11]: the last complete device call (both passes, the scan
 * and the read of the count between them). */
#define LP_SEL_OK       (1u << LP_LINE_OK)
#define LP_SEL_BAD      (1u << LP_LINE_BAD)
#define LP_SEL_FALLBACK (1u << LP_LINE_FALLBACK)
int lp_result_select(lp_handle *h, const lp_result *r, int64_t first, int64_t count, uint32_t status_mask,
                     int64_t *rows, uint64_t rows_cap, uint64_t *rows_len);

/* lp_result_select_where: lp_result_select with a predicate on the lines'
 * VALUES -- "status >= 500", "the path starts with /api/", "the user agent
 * contains bot", "the raw line contains a marker" -- evaluated on the device
 * without building a column; its row list is what the *_rows calls take.
 *
 * Line i of [first, first+count) is selected when its status is in
 * status_mask AND the predicate holds on the row lp_result_table_rows would
 * build for line i and the terms' (path, kind) columns.  The value of a term
 * is exactly that column's value on that row: the last delivery wins (the
 * earlier one when the later is null); a LONG taken from text is
 * Long.parseLong of it and null when that fails; a STRING taken from a long is
 * its decimal text; dates, times, month names and binary IPs are their
 * formatted text; a raw query string has its leading '&'.  A BAD or FALLBACK
 * line has only null values -- except in the pseudo-columns, valid for every
 * line as in the table: "@line" is STRING, "@offset", "@lineno" and "@status"
 * are LONG.  path is a requested "TYPE:path", a wildcard's member by its full
 * path, or a pseudo-column; kind (LP_CAST_LONG or LP_CAST_STRING) is the
 * column type the value is taken as.
 *
 * Ops: IS_NULL and EQ for either kind; LT / LE / GT / GE (value <op> lo) and
 * BETWEEN (lo <= value <= hi; lo > hi matches nothing) for LONG, EQ against
 * lo; PREFIX / SUFFIX / CONTAINS, and EQ, bytewise against str[0, str_len)
 * for STRING.  An empty operand: PREFIX, SUFFIX and CONTAINS are true on every
 * non-null value, EQ on the empty string only (an empty string is not null).
 *
 * Two-valued logic -- NOT SQL's three-valued one: a comparison with a null
 * value is false; IS_NULL is true exactly on null; LP_WHERE_NEGATE, or-ed
 * into op, flips the term's outcome after that rule, so a negated comparison
 * is TRUE on null and "is not null" is IS_NULL | NEGATE.  SQL's "<>" (false
 * on null) is EQ | NEGATE in one group and IS_NULL | NEGATE in another.
 *
 * The result is the AND over the groups of the OR over each group's terms
 * (group: non-decreasing over the array).  n_terms == 0 selects what
 * lp_result_select selects, by its code.
 *
 * Output, size protocol (*rows_len always set; LP_E_NOMEM with nothing
 * written), window, state, memory-kind checks and their codes: those of
 * lp_result_select, one implementation.  Additionally LP_E_INVALID: n_terms
 * outside 0..LP_WHERE_MAX_TERMS (or null terms with n_terms > 0), a null
 * path, a kind other than LONG / STRING, a kind the path's lp_casts lack or
 * the wrong one for a pseudo-column, an unknown op or one that does not exist
 * for the kind, a decreasing group, str_len outside 0..255 or a null str with
 * str_len > 0, or names and operands that together exceed the device table's
 * name pool (2048 bytes: the parameter / cookie names of the terms' paths
 * plus every STRING operand); LP_E_MISSING: a path the handle does not
 * deliver; on a device view LP_E_UNSUPPORTED: a path the device table does
 * not derive (lp_result_table's rule), or a handle without a device program.
 * On a host copy (with the input) the same call evaluates the host replay's
 * values, those of lp_result_table there, and gives the identical row list.
 * lp_last_timing [18] / [19]: the last complete device call with terms. */
#define LP_WHERE_MAX_TERMS 8
#define LP_WHERE_IS_NULL   0
#define LP_WHERE_EQ        1
#define LP_WHERE_LT        2
#define LP_WHERE_LE        3
#define LP_WHERE_GT        4
#define LP_WHERE_GE        5
#define LP_WHERE_BETWEEN   6
#define LP_WHERE_PREFIX    7
#define LP_WHERE_SUFFIX    8
#define LP_WHERE_CONTAINS  9
#define LP_WHERE_NEGATE    0x100
typedef struct lp_where_term {
    const char *path;
    int32_t kind;       /* LP_CAST_LONG or LP_CAST_STRING */
    int32_t op;         /* LP_WHERE_*, LP_WHERE_NEGATE may be or-ed in */
    int32_t group;      /* terms of one group are OR-ed, the groups AND-ed */
    int32_t str_len;    /* STRING operand, 0..255 bytes */
    int64_t lo, hi;     /* LONG operands */
    const uint8_t *str;
} lp_where_term;
int lp_result_select_where(lp_handle *h, const lp_result *r, int64_t first, int64_t count, uint32_t status_mask,
                           const lp_where_term *terms, int n_terms, int64_t *rows, uint64_t rows_cap,
                           uint64_t *rows_len);

/* lp_result_table / lp_result_table_map with row k = line rows[k] (batch-
 * relative, as lp_result_select writes them): what the record reader and the
 * SerDe hand on (ApacheHttpdLogfileRecordReader.java:246-287,
 * ApacheHttpdlogDeserializer.java:284-291) when rows holds the OK lines.  The
 * indices may come in any order and may repeat (a gather); n_rows may be 0.
 * Every output array has n_rows (or n_rows + 1) elements, exactly as with
 * count; return codes and the LP_E_NOMEM / chars_len protocol are those of
 * the window calls, which are the same implementation with row k = line
 * first + k.  A row that names a BAD or FALLBACK line is valid 0.  rows is
 * host memory on a host copy -- an index outside [0, n_lines) returns
 * LP_E_INVALID before anything is written -- and device memory of the
 * handle's device on a device view (anything else: LP_E_INVALID), where the
 * kernels check each index: one outside the batch is never dereferenced, its
 * row is valid 0 and the call returns LP_E_INVALID.
 *
 * Pseudo-columns: lp_table_col.path of lp_result_table and
 * lp_result_table_rows (both modes) may also be one of four names without a
 * ':' (so none collides with a "TYPE:path"), valid for EVERY row whatever the
 * line's status, and needing no lp_casts entry:
 *   "@line"   STRING only: the line's raw bytes, input[line_off[i],
 *             line_off[i+1] - 1) less the '\r' of a "\r\n" terminator (the
 *             parse kernels' line; right for a final line without terminator).
 *             Not validated: a FALLBACK line may hold invalid UTF-8 or be
 *             longer than 8191 bytes;
 *   "@offset" LONG only: line_off[i], the batch-relative LongWritable key
 *             (ApacheHttpdLogfileRecordReader.java:283-287);
 *   "@lineno" LONG only: lp_result.first_line + i;
 *   "@status" LONG only: LP_LINE_*.
 * Any other kind for them gives LP_E_INVALID.  On a device view of a handle
 * without a device program (every line FALLBACK) they are LP_E_UNSUPPORTED as
 * every column is: build them from a host copy. */
int lp_result_table_rows(lp_handle *h, const lp_result *r, const int64_t *rows, int64_t n_rows,
                         lp_table_col *cols, int n_cols, int threads);
int lp_result_table_map_rows(lp_handle *h, const lp_result *r, const int64_t *rows, int64_t n_rows,
                             lp_table_map_col *cols, int n_cols, int threads);

/* ---- Dictionary-encoded STRING columns (Arrow dictionary<int32, utf8>). ----
 * A log table's bytes are almost all strings from small value sets (method,
 * protocol, status, host, user agent, referer, path).  The consumers' string
 * types all have a dictionary form -- Arrow's DictionaryArray, ORC's
 * DICTIONARY_V2 string encoding, Parquet's RLE_DICTIONARY -- which takes a
 * 4-byte index per row and each distinct value once.  These calls build that
 * form directly: the plain column's bytes are never written.  The gain is the
 * output's size for a repetitive column, not the call's time: on a device
 * view it takes longer than lp_result_table of the same path, and a column of
 * nearly all distinct values comes out larger too.
 *
 * path: any path lp_result_table accepts with kind LP_CAST_STRING on this
 * view, "@line" included.  Rows as lp_result_table (first, count) /
 * lp_result_table_rows (rows, n_rows).  Exactly:
 *   valid[k]  byte for byte what lp_result_table writes for the path as a
 *             STRING column over the same rows;
 *   index[k]  for a valid row, the dictionary entry whose bytes equal that
 *             plain column's value of row k; 0 for a row that is not valid
 *             (a null contributes no entry; "" is a value and gets one);
 *   dict_off  [dict_len + 1] Arrow offsets into dict_chars: entry j is
 *             dict_chars[dict_off[j], dict_off[j + 1]).
 * Entries are pairwise distinct and ordered by FIRST OCCURRENCE: entry j is
 * the value whose first valid row comes j-th, counting the call's row index
 * k (with a row list that repeats or runs backwards the order follows k, not
 * the line number).  The result is therefore deterministic, and a host copy
 * and a device view give identical index, dict_off and dict_chars.
 * Sizes as chars_cap / chars_len: every call sets dict_len (distinct values
 * among the valid rows) and dict_chars_len (their bytes); when dict_cap <
 * dict_len or dict_chars_cap < dict_chars_len the call returns LP_E_NOMEM with
 * both lengths exact, nothing is written past either capacity, and the other
 * outputs are unspecified: call again.  dict_off has room for dict_cap + 1
 * words and is never NULL.
 * Errors: count (n_rows) above 2^31 - 1 is LP_E_INVALID; the others are those
 * of lp_result_table / lp_result_table_rows (a row index outside the batch,
 * LP_E_UNSUPPORTED for a path the device table does not derive,
 * LP_E_MISSING).  On a device view every pointer and the row list are memory
 * of the handle's device (anything else: LP_E_INVALID, nothing dereferenced),
 * and the column is built in HBM by a lock-free hash kernel; on a
 * host copy it is built from the host table and a hash map, `threads` as in
 * lp_result_table.  LP_E_DEVICE if the device's hash table overflowed (it
 * cannot: it has two slots per row).  lp_last_timing [12..15]: the last
 * device call's phases, summed over its columns. */
typedef struct lp_table_dict_col {
    const char *path;
    uint8_t *valid;          /* [count] */
    int32_t *index;          /* [count] */
    int64_t *dict_off;       /* [dict_cap + 1] */
    char    *dict_chars;     /* dict_chars_cap bytes */
    int64_t  dict_cap;       /* in:  entries dict_off has room for */
    uint64_t dict_chars_cap; /* in */
    int64_t  dict_len;       /* out: distinct values among the valid rows */
    uint64_t dict_chars_len; /* out: bytes of the dictionary's values */
} lp_table_dict_col;
int lp_result_table_dict(lp_handle *h, const lp_result *r, int64_t first, int64_t count, lp_table_dict_col *cols,
                         int n_cols, int threads);
int lp_result_table_dict_rows(lp_handle *h, const lp_result *r, const int64_t *rows, int64_t n_rows,
                              lp_table_dict_col *cols, int n_cols, int threads);

/* ---- Grouped aggregates (GROUP BY) over the rows of a batch. ----
 * What the reference's users run on top of the parser is a query over log
 * lines: the Hive SerDe hands Hive one row per line (httpdlog-serde/.../
 * ApacheHttpdlogDeserializer.java:284-323), the record reader one ParsedRecord
 * (ApacheHttpdLogfileRecordReader.java:246-287), the Pig loader one tuple
 * (httpdlog-pigloader/.../Loader.java:227-229), and after WHERE nearly every
 * such query ends in GROUP BY: hits and bytes per status, top paths, requests
 * per client or per hour.  These calls answer it from the parsed batch: the
 * groups of up to LP_GROUP_MAX_KEYS key columns and up to LP_GROUP_MAX_AGGS
 * aggregates of LONG measures per group, without building a key or measure
 * column -- a handful of rows out instead of 12 bytes per row and an
 * aggregation elsewhere.
 *
 * Rows: those of lp_result_table (first, count) / lp_result_table_rows (rows,
 * n_rows: any order, repeats allowed; lp_result_select_where's output goes
 * straight in).  The value of a key or a measure on row k is exactly what
 * lp_result_table_rows builds for its (path, kind): the last delivery wins,
 * a LONG from text is Long.parseLong or null, dates and times are their
 * formatted text, CLF2NUM gives 0 for "-", and the pseudo-columns "@line" /
 * "@offset" / "@lineno" / "@status" are valid for every status while a BAD or
 * FALLBACK line is null in every real column.  Measures are LONG (a DOUBLE
 * sum would depend on the order of arrival).
 *
 * Keys: two rows are in one group when every key agrees -- both null, or both
 * non-null and equal: by int64 value for a LONG key ("007" and "7" are one
 * group), by bytes for a STRING key (they are two).  Null is a key value of
 * its own, distinct from "".  n_keys == 0: one group of every row (none when
 * count is 0).
 *
 * Output: groups are numbered by FIRST OCCURRENCE over the call's row index k,
 * as dictionary entries are.  rep[g] is the batch-relative line of group g's
 * first row: lp_result_table_rows(rep) gives the key values; no key bytes are
 * written here.  group_of[k] (optional) is row k's group.  Aggregate a writes
 * value[g] / valid[g]: COUNT_ROWS and COUNT are always valid; SUM (two's-
 * complement wrap, Java's long +), MIN and MAX of the non-null values are
 * valid 0, value 0, for a group without one.  Every result is independent of
 * the order the rows are taken in, so a device view and a host copy give
 * byte-identical rep, group_of, value and valid.
 * Sizes: rep and every value / valid have groups_cap entries; n_groups is
 * always set and exact; groups_cap < n_groups returns LP_E_NOMEM with rep,
 * value and valid untouched (group_of is unspecified then): call again.
 * count 0: LP_OK, n_groups 0.
 * Errors: those of lp_result_table / lp_result_table_rows through the same
 * checks (LP_E_MISSING, LP_E_UNSUPPORTED on a device view for a path the
 * device table does not derive, LP_E_STATE, a row index outside the batch);
 * LP_E_INVALID additionally for n_keys outside 0..LP_GROUP_MAX_KEYS or n_aggs
 * outside 0..LP_GROUP_MAX_AGGS, a null array with a count above 0, a null
 * path where one is needed or a path on COUNT_ROWS, a key kind other than
 * LONG / STRING or one the path's lp_casts lack, a measure whose lp_casts lack
 * LONG, an unknown op, a null value / valid or rep with groups_cap > 0, a
 * negative groups_cap, names that exceed the device table's pool, and count
 * above 2^31 - 1.  On a device view every pointer and the row list are memory
 * of the handle's device (anything else: LP_E_INVALID, nothing dereferenced),
 * and the groups are built in HBM: the dictionary's lock-free insert on a
 * hash of the key tuple, then an accumulation in per-block LDS copies (few
 * groups) or with global atomics after a wave-level merge of the leading
 * groups; LP_E_DEVICE if the hash table overflowed (it
 * cannot: it has two slots per row).  On a host copy (with the input) they are
 * built from the host table's columns and a hash map in row order, `threads`
 * as in lp_result_table.  Groups of several batches or GPUs are merged by the
 * caller, by key value, on these few rows.
 * lp_last_timing [20..22]: the last complete device call's phases. */
#define LP_GROUP_MAX_KEYS 4
#define LP_GROUP_MAX_AGGS 8
#define LP_AGG_COUNT_ROWS 0   /* path NULL: the group's rows */
#define LP_AGG_COUNT      1   /* rows on which the path's LONG value is not null */
#define LP_AGG_SUM        2   /* of the non-null values, two's-complement wrap (Java long +) */
#define LP_AGG_MIN        3
#define LP_AGG_MAX        4
typedef struct lp_group_key {
    const char *path;
    int32_t kind;        /* LP_CAST_LONG or LP_CAST_STRING */
} lp_group_key;
typedef struct lp_group_agg {
    const char *path;    /* NULL for LP_AGG_COUNT_ROWS */
    int32_t op;          /* LP_AGG_* */
    int64_t *value;      /* [groups_cap] */
    uint8_t *valid;      /* [groups_cap] */
} lp_group_agg;
typedef struct lp_group_out {
    int64_t *rep;        /* [groups_cap] batch-relative line of the group's first row */
    int32_t *group_of;   /* [count] group of row k; may be NULL */
    int64_t  groups_cap; /* in */
    int64_t  n_groups;   /* out, always set */
} lp_group_out;
int lp_result_group(lp_handle *h, const lp_result *r, int64_t first, int64_t count, const lp_group_key *keys,
                    int n_keys, const lp_group_agg *aggs, int n_aggs, lp_group_out *out, int threads);
int lp_result_group_rows(lp_handle *h, const lp_result *r, const int64_t *rows, int64_t n_rows,
                         const lp_group_key *keys, int n_keys, const lp_group_agg *aggs, int n_aggs,
                         lp_group_out *out, int threads);

/* ---- Arrow C Data Interface export of the typed, dictionary and map columns. ----
 * One call turns rows of a batch into an Arrow record batch that any Arrow
 * consumer imports as it is (Arrow Java's Data.importVectorSchemaRoot,
 * pyarrow's RecordBatch._import_from_c, the ORC / Parquet writers): the
 * columns the Hadoop ParsedRecord holds per line and the Hive SerDe reads
 * back (httpdlog-inputformat/.../ParsedRecord.java:154-214,
 * httpdlog-serde/.../ApacheHttpdlogDeserializer.java:224-240, 295-323) and
 * the ".*" map the record reader registers and the Pig Loader returns
 * (ApacheHttpdLogfileRecordReader.java:206-208, httpdlog-pigloader/.../
 * Loader.java:227-229), with what Arrow wants and the table calls above do
 * not give: validity BITMAPS with exact null counts, int32 map offsets, the
 * nested struct / map / dictionary tree, and a lifetime of their own.
 *
 * The three structures are the Arrow specification's, under its guards: a
 * consumer that also includes Arrow's abi.h sees no redefinition. */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
    const char *format;
    const char *name;
    const char *metadata;
    int64_t flags;
    int64_t n_children;
    struct ArrowSchema **children;
    struct ArrowSchema *dictionary;
    void (*release)(struct ArrowSchema *);
    void *private_data;
};
struct ArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void **buffers;
    struct ArrowArray **children;
    struct ArrowArray *dictionary;
    void (*release)(struct ArrowArray *);
    void *private_data;
};
#endif
#ifndef ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_C_DEVICE_DATA_INTERFACE
typedef int32_t ArrowDeviceType;
#define ARROW_DEVICE_CPU 1
#define ARROW_DEVICE_ROCM 10
struct ArrowDeviceArray {
    struct ArrowArray array;
    int64_t device_id;
    ArrowDeviceType device_type;
    void *sync_event;
    int64_t reserved[3];
};
#endif

/* A column of lp_result_arrow.  The layout (offset 0 everywhere; the top level
 * a non-nullable struct "+s" of `length` rows, one child per column in the
 * order given):
 *   PLAIN LONG    "l"  validity, the i64 values                       nullable
 *   PLAIN DOUBLE  "g"  validity, the f64 values                       nullable
 *   PLAIN STRING  "U"  (large_utf8) validity, the int64 offsets as the table
 *                      writes them (no narrowing, no copy), chars     nullable
 *   "@line"       "Z"  (large_binary: its bytes are not validated UTF-8)
 *   DICT          "i"  validity, index; nullable; dictionary = a non-nullable
 *                      "U" array of dict_len entries (dict_off, dict_chars);
 *                      ARROW_FLAG_DICTIONARY_ORDERED not set
 *   MAP           "+m" validity, int32 offsets [rows + 1] NARROWED from
 *                      entry_off; nullable; ARROW_FLAG_MAP_KEYS_SORTED not set;
 *                      one child "entries" ("+s", not nullable, entries_len
 *                      long) of "key" ("U", not nullable: key_off / key_chars)
 *                      and "value" ("U", nullable, null_count 0, no bitmap:
 *                      val_off / val_chars)
 * Validity is Arrow's bitmap: bit k & 7 of byte k >> 3 is set when the table's
 * valid[k] != 0, every bit at or past `length` is 0, the allocation a multiple
 * of 64 bytes; null_count is always exact (never -1); a column without nulls
 * has a NULL validity pointer and no bitmap (the dense table of the OK lines
 * costs nothing). */
#define LP_ARROW_PLAIN 0   /* kind = LP_CAST_STRING / LP_CAST_LONG / LP_CAST_DOUBLE */
#define LP_ARROW_DICT  1   /* lp_result_table_dict's column */
#define LP_ARROW_MAP   2   /* lp_result_table_map's column (a ".*" path) */
typedef struct lp_arrow_col {
    const char *path;      /* as the table calls take it, pseudo-columns included */
    const char *name;      /* Arrow field name; NULL: the path */
    int32_t form;          /* LP_ARROW_* */
    int32_t kind;          /* LP_ARROW_PLAIN only */
} lp_arrow_col;

/* The rows of a batch as an Arrow record batch.  rows == NULL: the window
 * [first, first+count); else row k = line rows[k] (n_rows in count, first
 * ignored), exactly as the *_rows calls.  From a host copy array_out->array is
 * an importable ArrowArray in malloc'ed memory (device_type ARROW_DEVICE_CPU,
 * device_id -1); on a device view every buffer is hipMalloc'ed memory of the
 * handle's device (ARROW_DEVICE_ROCM, device_id the handle's device) and the
 * bitmaps, null counts and int32 offsets are made by kernels.  sync_event is
 * NULL: the call returns after its stream is synchronised, as the table calls
 * do, so the buffers are complete when it returns.
 * The call allocates every buffer itself and runs the tables' LP_E_NOMEM size
 * protocol inside; the batch belongs to the consumer until it calls the
 * release callbacks and OUTLIVES the handle's next batch and the handle.
 * Errors: n_cols == 0, an unknown form, or a map with more than 2^31 - 1
 * entries (build it in windows) is LP_E_INVALID; every other code is the
 * underlying table call's, unchanged (LP_E_MISSING, LP_E_UNSUPPORTED,
 * LP_E_INVALID, LP_E_STATE, a row index outside the batch).  On any error both
 * outputs are released (release == NULL) and nothing leaks.  count == 0 gives
 * valid zero-length arrays whose offsets buffers hold the single 0.
 * lp_last_timing [16]: the last device export's packaging kernels. */
int lp_result_arrow(lp_handle *h, const lp_result *r, const int64_t *rows, int64_t first, int64_t count,
                    const lp_arrow_col *cols, int n_cols, int threads, struct ArrowSchema *schema_out,
                    struct ArrowDeviceArray *array_out);

/* The packaging alone, without a handle: wrap columns that table calls (or
 * anything else) already filled, n_rows rows each.  device < 0: host memory;
 * else memory of that device, and stream (a hipStream_t, NULL = the default
 * stream) carries the kernels; the call returns after synchronising it.
 * Children: the plain columns, then the dictionary columns, then the maps.
 * A column's Arrow field name is *_names[i], or its path when the names array
 * or the entry is NULL.  Of a column only its arrays, kind and lengths
 * (chars_len, dict_len, entries_len, ...) are read; valid may have any
 * alignment.
 * It WRAPS: no value buffer is copied.  It allocates the bitmaps, the narrowed
 * map offsets and the structures, and frees exactly those on release.
 * owner->free_fn(owner->ctx) is called exactly once, when the last exported
 * ARRAY structure has been released (the record batch, any child or
 * dictionary the consumer moved out of it); the schema holds no buffer and
 * releases independently, in either order.  owner may be NULL.  When the call
 * fails the owner is NOT called: the buffers stay the caller's.
 * The release callbacks follow the specification: a child the consumer moved
 * out (its release NULL) is skipped, release is set to NULL last, and
 * private_data is ours. */
typedef struct lp_arrow_owner {
    void (*free_fn)(void *ctx);
    void *ctx;
} lp_arrow_owner;
int lp_arrow_from_tables(int device, void *stream, int64_t n_rows,
                         const lp_table_col *plain, const char *const *plain_names, int n_plain,
                         const lp_table_dict_col *dict, const char *const *dict_names, int n_dict,
                         const lp_table_map_col *map, const char *const *map_names, int n_map,
                         const lp_arrow_owner *owner, struct ArrowSchema *schema_out,
                         struct ArrowDeviceArray *array_out);

/* Deep copy of a record batch of the types above to host memory, for a
 * consumer whose Arrow build has no ROCm memory manager (pyarrow among them).
 * `in` stays the caller's to release; `out` is an independent ArrowArray of
 * malloc'ed buffers.  LP_E_INVALID for a format this library does not export. */
int lp_arrow_to_host(const struct ArrowSchema *schema, const struct ArrowDeviceArray *in, struct ArrowArray *out);

/* Description of the compiled device program (for logs/tests), NUL-terminated. */
int64_t lp_describe(lp_handle *h, char *out, size_t cap);

/* Synthetic 'combined' access-log generator (deterministic per seed), used
 * by bench.py and tests to build BASELINE.json config-2 inputs.  Writes
 * complete lines into out (cap bytes) starting at line index first_line;
 * returns bytes written and sets *n_lines. */
int64_t lp_synth_combined(uint64_t seed, int64_t first_line, int64_t max_lines,
                          char *out, size_t cap, int64_t *n_lines);

/* The same for each BASELINE.json workload:
 *   LP_SYNTH_COMBINED  config 2, 'combined'
 *   LP_SYNTH_STRFTIME  config 3, '%h %l %u [%{%d/%b/%Y %T}t.%{msec_frac}t] "%r" %>s %b
 *                      "%{Referer}i" "%{User-Agent}i" %I %O', 5 % malformed lines
 *   LP_SYNTH_NGINX     config 4, the NGINX log_format of
 *                      hpt/nginxmodules/NginxUpstreamTest.java:94
 *   LP_SYNTH_MIXED     config 5, 40 % config-2, 30 % config-4 and 30 % 'common'
 *                      lines (mutually exclusive formats), chosen per line
 * Returns LP_E_INVALID for an unknown workload. */
#define LP_SYNTH_COMBINED 2
#define LP_SYNTH_STRFTIME 3
#define LP_SYNTH_NGINX 4
#define LP_SYNTH_MIXED 5
int64_t lp_synth(int workload, uint64_t seed, int64_t first_line, int64_t max_lines,
                 char *out, size_t cap, int64_t *n_lines);

#ifdef __cplusplus
}
#endif
#endif
