"""logparser_amd -- MI355X-native batch engine for logparser's per-line hot path.

Host-side mirror of the reference's parser surface for this path
(nl.basjes.parse.httpdlog.HttpdLoglineParser / nl.basjes.parse.core.Parser,
reference: httpdlog/httpdlog-parser/src/main/java/nl/basjes/parse/httpdlog/
HttpdLoglineParser.java:44-126 and parser-core/src/main/java/nl/basjes/parse/core/
Parser.java:496-756, 904-1012) over the C ABI in include/logparser_amd.h.

    parser = HttpdLoglineParser("combined", ["TIME.EPOCH:request.receive.time.epoch", ...])
    batch  = parser.parse_batch(raw_bytes_or_cuda_uint8_tensor)   # all lines on the GPU
    batch.status            # per line: OK / BAD (DissectionFailure) / FALLBACK
    batch.record(i)         # {"TYPE:path": [values]} as the reference setters receive them
    parser.parse(line)      # Parser.parse(line) for one line (raises DissectionFailure)

The engine runs only on the GPU: there is no CPU implementation behind this
module, and every call fails loudly when the HIP library or a device is
missing.  FALLBACK lines are the lines the device could not prove it handles
exactly; a deployment hands them to the reference Java dissector.
"""
import ctypes
import json
import os

import numpy as np

from .setters import (CAST_DOUBLE, CAST_LONG, CAST_STRING, NO_CASTS, STRING_ONLY, STRING_OR_DOUBLE,  # noqa: F401
                      STRING_OR_LONG, STRING_OR_LONG_OR_DOUBLE, FatalErrorDuringCallOfSetterMethod, SetterPolicy,
                      Target, cleanup_field_value, deliver)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LOGPARSER_AMD_LIB") or os.path.join(_HERE, "_lib", "liblogparser_amd.so")

LP_OK, LP_E_INVALID, LP_E_MISSING, LP_E_UNSUPPORTED, LP_E_DEVICE, LP_E_NOMEM, LP_E_STATE = 0, -1, -2, -3, -4, -5, -6
LINE_OK, LINE_BAD, LINE_FALLBACK = 0, 1, 2
BUF_HOST, BUF_DEVICE = 0, 1
OPT_FORCE_DIRECT, OPT_MAX_RETRIES, OPT_ARENA_BYTES, OPT_CHUNK_LINES, OPT_CHUNK_WAIT, OPT_ONE_PASS = 1, 2, 3, 4, 5, 6
OPT_FIXED_SHAPE = 7  # 0: never the chunk kernel's fixed-shape instances (default 1)
OPT_DICT_HASH_BITS = 8  # tests: low bits of a value's hash the device dictionary keeps for its home slot (0: all)
OPT_GROUP_LDS_WORDS = 9  # tests, measurements: LDS budget (8-byte words) of the device group call's privatised regime (0: default, -1: none)
OPT_GROUP_PEEL = 10  # measurements: peel rounds of its global-atomic regime (0: default, -1: none)
ARENA_SHARDS = 64
# lp_result_select's status mask (1 << LINE_*)
SEL_OK, SEL_BAD, SEL_FALLBACK = 1 << LINE_OK, 1 << LINE_BAD, 1 << LINE_FALLBACK
# the device select's tiles in lines (csrc/kernels.h SEL_WAVE_LINES / SEL_BLOCK_LINES: one lane takes 16 lines)
SEL_WAVE_LINES, SEL_BLOCK_LINES = 1024, 4096
# the pseudo-columns of lp_result_table / lp_result_table_rows: valid for every row whatever its status
PSEUDO_COLUMNS = {"@line": str, "@offset": int, "@lineno": int, "@status": int}


class LpColumn(ctypes.Structure):
    """lp_column (include/logparser_amd.h)"""
    _fields_ = [("name", ctypes.c_char * 16), ("index", ctypes.c_int32), ("elem_size", ctypes.c_int32),
                ("offset", ctypes.c_uint64)]


EMIT_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
                           ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint32, ctypes.c_int64)
VALUE_STRING, VALUE_NULL, VALUE_LONG = 0, 1, 2


class LpTableCol(ctypes.Structure):
    _fields_ = [("path", ctypes.c_char_p), ("kind", ctypes.c_int32), ("valid", ctypes.c_void_p),
                ("i64", ctypes.c_void_p), ("f64", ctypes.c_void_p), ("chars", ctypes.c_void_p),
                ("chars_cap", ctypes.c_uint64), ("chars_len", ctypes.c_uint64)]


class LpWhereTerm(ctypes.Structure):
    """lp_where_term (include/logparser_amd.h): one term of lp_result_select_where"""
    _fields_ = [("path", ctypes.c_char_p), ("kind", ctypes.c_int32), ("op", ctypes.c_int32), ("group", ctypes.c_int32),
                ("str_len", ctypes.c_int32), ("lo", ctypes.c_int64), ("hi", ctypes.c_int64), ("str", ctypes.c_char_p)]


# lp_result_select_where's ops (LP_WHERE_*); WHERE_NEGATE may be or-ed in
(WHERE_IS_NULL, WHERE_EQ, WHERE_LT, WHERE_LE, WHERE_GT, WHERE_GE, WHERE_BETWEEN, WHERE_PREFIX, WHERE_SUFFIX,
 WHERE_CONTAINS) = range(10)
WHERE_NEGATE = 0x100
WHERE_MAX_TERMS = 8
_WHERE_LONG_OPS = (WHERE_IS_NULL, WHERE_EQ, WHERE_LT, WHERE_LE, WHERE_GT, WHERE_GE, WHERE_BETWEEN)
_WHERE_STRING_OPS = (WHERE_IS_NULL, WHERE_EQ, WHERE_PREFIX, WHERE_SUFFIX, WHERE_CONTAINS)


class Where:
    """One term of BatchResult.select_where_*: `path` (a requested "TYPE:path",
    a wildcard's member, or a pseudo-column) taken as a column of `kind` (int:
    BIGINT, str: STRING) against an operand.  kind defaults from the
    operand's Python type -- int gives int, str / bytes give str -- and is
    required for WHERE_IS_NULL, which has no operand.  op: WHERE_*; value: the
    operand (BETWEEN: value <= x <= hi); terms of one group are OR-ed, the
    groups AND-ed; negate flips the term's outcome (true on null then: the
    logic is two-valued).  Argument errors raise here, before any engine call."""

    def __init__(self, path, op, value=None, hi=None, kind=None, group=0, negate=False):
        if not isinstance(path, str) or not path:
            raise ValueError("Where: path must be a non-empty str")
        if op not in range(10):
            raise ValueError("Where: unknown op %r" % (op,))
        if isinstance(value, bool) or isinstance(hi, bool):
            raise TypeError("Where: a bool is no operand")
        if kind is None:
            if isinstance(value, int):
                kind = int
            elif isinstance(value, (str, bytes)):
                kind = str
            else:
                raise ValueError("Where: kind is required when the operand does not give it (IS_NULL)")
        if kind not in (int, str):
            raise ValueError("Where: kind must be int or str")
        if op not in (_WHERE_LONG_OPS if kind is int else _WHERE_STRING_OPS):
            raise ValueError("Where: op %d does not exist for a %s column" % (op, "BIGINT" if kind is int else "STRING"))
        if op == WHERE_IS_NULL:
            if value is not None or hi is not None:
                raise ValueError("Where: IS_NULL takes no operand")
        elif kind is int:
            if not isinstance(value, int) or (op == WHERE_BETWEEN) != (hi is not None) or \
                    (hi is not None and not isinstance(hi, int)):
                raise ValueError("Where: a BIGINT op takes an int (BETWEEN: value and hi)")
            for x in (value, hi or 0):
                if not -(1 << 63) <= x < (1 << 63):
                    raise ValueError("Where: operand outside int64")
        else:
            if not isinstance(value, (str, bytes)) or hi is not None:
                raise ValueError("Where: a STRING op takes one str / bytes operand")
            value = value.encode("utf-8") if isinstance(value, str) else bytes(value)
            if len(value) > 255:
                raise ValueError("Where: a STRING operand has at most 255 bytes")
        if not isinstance(group, int) or group < 0:
            raise ValueError("Where: group must be an int >= 0")
        self.path, self.op, self.value, self.hi, self.kind, self.group, self.negate = (path, op, value, hi, kind, group,
                                                                                       bool(negate))

    def __repr__(self):
        return "Where(%r, %d, %r, hi=%r, kind=%s, group=%d, negate=%r)" % (self.path, self.op, self.value, self.hi,
                                                                            self.kind.__name__, self.group, self.negate)


class LpGroupKey(ctypes.Structure):
    """lp_group_key (include/logparser_amd.h)"""
    _fields_ = [("path", ctypes.c_char_p), ("kind", ctypes.c_int32)]


class LpGroupAgg(ctypes.Structure):
    """lp_group_agg (include/logparser_amd.h)"""
    _fields_ = [("path", ctypes.c_char_p), ("op", ctypes.c_int32), ("value", ctypes.c_void_p), ("valid", ctypes.c_void_p)]


class LpGroupOut(ctypes.Structure):
    """lp_group_out (include/logparser_amd.h)"""
    _fields_ = [("rep", ctypes.c_void_p), ("group_of", ctypes.c_void_p), ("groups_cap", ctypes.c_int64),
                ("n_groups", ctypes.c_int64)]


# lp_result_group's aggregates (LP_AGG_*) and limits
AGG_COUNT_ROWS, AGG_COUNT, AGG_SUM, AGG_MIN, AGG_MAX = range(5)
GROUP_MAX_KEYS, GROUP_MAX_AGGS = 4, 8
# the device call's default LDS budget in 8-byte words (csrc/lp_group.h GROUP_LDS_WORDS)
GROUP_LDS_WORDS = 4096


class Agg:
    """One aggregate of BatchResult.group_*: AGG_COUNT_ROWS (no path: the
    group's rows), or AGG_COUNT / AGG_SUM / AGG_MIN / AGG_MAX of `path` (a
    requested "TYPE:path", a wildcard's member, or a LONG pseudo-column) taken
    as a BIGINT column: the rows on which it is not null, and the wrapping
    sum, the least and the greatest of those values.  Argument errors raise
    here, before any engine call."""

    def __init__(self, op, path=None):
        if isinstance(op, bool) or not isinstance(op, int) or op not in range(5):
            raise ValueError("Agg: unknown op %r" % (op,))
        if op == AGG_COUNT_ROWS:
            if path is not None:
                raise ValueError("Agg: AGG_COUNT_ROWS takes no path")
        elif not isinstance(path, str) or not path:
            raise ValueError("Agg: path must be a non-empty str")
        self.op, self.path = op, path

    def __repr__(self):
        return "Agg(%d, %r)" % (self.op, self.path)


def group_acc_words(aggs):
    """accumulator words per group of a list of Agg (csrc/lp_group.h): the
    rows, one non-null count per distinct measure, one per SUM / MIN / MAX"""
    return 1 + len({a.path for a in aggs if a.path is not None}) + sum(1 for a in aggs if a.op >= AGG_SUM)


def _group_args(keys, aggs):
    """(lp_group_key array or None, lp_group_agg array or None) of [(path, str | int)] and a list of Agg"""
    keys, aggs = list(keys), list(aggs)
    if len(keys) > GROUP_MAX_KEYS:
        raise ValueError("at most %d keys" % GROUP_MAX_KEYS)
    if len(aggs) > GROUP_MAX_AGGS:
        raise ValueError("at most %d aggregates" % GROUP_MAX_AGGS)
    if any(not isinstance(a, Agg) for a in aggs):
        raise TypeError("aggs: Agg objects expected")
    for k in keys:
        if not (isinstance(k, tuple) and len(k) == 2 and isinstance(k[0], str) and k[0] and k[1] in (int, str)):
            raise ValueError("keys: (path, str | int) pairs expected")
    karr = (LpGroupKey * len(keys))() if keys else None
    for j, (path, typ) in enumerate(keys):
        karr[j].path = path.encode()
        karr[j].kind = CAST_LONG if typ is int else CAST_STRING
    aarr = (LpGroupAgg * len(aggs))() if aggs else None
    for j, a in enumerate(aggs):
        aarr[j].path = a.path.encode() if a.path is not None else None
        aarr[j].op = a.op
    return karr, aarr


def _where_array(terms):
    """(lp_where_term array or None, n, what must stay alive) of a list of Where"""
    terms = list(terms)
    if len(terms) > WHERE_MAX_TERMS:
        raise ValueError("at most %d terms" % WHERE_MAX_TERMS)
    if any(not isinstance(t, Where) for t in terms):
        raise TypeError("terms: Where objects expected")
    if any(a.group > b.group for a, b in zip(terms, terms[1:])):
        raise ValueError("terms: group must not decrease")
    if not terms:
        return None, 0, []
    arr = (LpWhereTerm * len(terms))()
    keep = []
    for k, t in enumerate(terms):
        w = arr[k]
        w.path = t.path.encode()
        w.kind = CAST_LONG if t.kind is int else CAST_STRING
        w.op = t.op | (WHERE_NEGATE if t.negate else 0)
        w.group = t.group
        if t.kind is int:
            w.lo, w.hi = t.value or 0, t.hi or 0
        elif t.value is not None:
            buf = ctypes.create_string_buffer(t.value, len(t.value) + 1)  # (operands may hold NUL bytes)
            keep.append(buf)
            w.str = ctypes.cast(buf, ctypes.c_char_p)
            w.str_len = len(t.value)
    return arr, len(terms), keep


class LpTableMapCol(ctypes.Structure):
    """lp_table_map_col (include/logparser_amd.h): one Arrow map<string,string> column"""
    _fields_ = [("path", ctypes.c_char_p), ("valid", ctypes.c_void_p), ("entry_off", ctypes.c_void_p),
                ("key_off", ctypes.c_void_p), ("val_off", ctypes.c_void_p), ("key_chars", ctypes.c_void_p),
                ("val_chars", ctypes.c_void_p), ("entries_cap", ctypes.c_uint64), ("key_chars_cap", ctypes.c_uint64),
                ("val_chars_cap", ctypes.c_uint64), ("entries_len", ctypes.c_uint64),
                ("key_chars_len", ctypes.c_uint64), ("val_chars_len", ctypes.c_uint64)]


class LpTableDictCol(ctypes.Structure):
    """lp_table_dict_col (include/logparser_amd.h): one Arrow dictionary<int32, utf8> column"""
    _fields_ = [("path", ctypes.c_char_p), ("valid", ctypes.c_void_p), ("index", ctypes.c_void_p),
                ("dict_off", ctypes.c_void_p), ("dict_chars", ctypes.c_void_p), ("dict_cap", ctypes.c_int64),
                ("dict_chars_cap", ctypes.c_uint64), ("dict_len", ctypes.c_int64), ("dict_chars_len", ctypes.c_uint64)]


class ArrowSchema(ctypes.Structure):
    """struct ArrowSchema of the Arrow C Data Interface (include/logparser_amd.h)"""


ArrowSchema._fields_ = [("format", ctypes.c_char_p), ("name", ctypes.c_char_p), ("metadata", ctypes.c_void_p),
                        ("flags", ctypes.c_int64), ("n_children", ctypes.c_int64),
                        ("children", ctypes.POINTER(ctypes.POINTER(ArrowSchema))),
                        ("dictionary", ctypes.POINTER(ArrowSchema)),
                        ("release", ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowSchema))),
                        ("private_data", ctypes.c_void_p)]


class ArrowArray(ctypes.Structure):
    """struct ArrowArray of the Arrow C Data Interface"""


ArrowArray._fields_ = [("length", ctypes.c_int64), ("null_count", ctypes.c_int64), ("offset", ctypes.c_int64),
                       ("n_buffers", ctypes.c_int64), ("n_children", ctypes.c_int64),
                       ("buffers", ctypes.POINTER(ctypes.c_void_p)),
                       ("children", ctypes.POINTER(ctypes.POINTER(ArrowArray))),
                       ("dictionary", ctypes.POINTER(ArrowArray)),
                       ("release", ctypes.CFUNCTYPE(None, ctypes.POINTER(ArrowArray))),
                       ("private_data", ctypes.c_void_p)]


class ArrowDeviceArray(ctypes.Structure):
    """struct ArrowDeviceArray of the Arrow C Device Data Interface"""
    _fields_ = [("array", ArrowArray), ("device_id", ctypes.c_int64), ("device_type", ctypes.c_int32),
                ("sync_event", ctypes.c_void_p), ("reserved", ctypes.c_int64 * 3)]


ARROW_FLAG_DICTIONARY_ORDERED, ARROW_FLAG_NULLABLE, ARROW_FLAG_MAP_KEYS_SORTED = 1, 2, 4
ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM = 1, 10
ARROW_PLAIN, ARROW_DICT, ARROW_MAP = 0, 1, 2
# the device validity kernel's tiles in rows (csrc/kernels.h ARROW_WAVE_ROWS / ARROW_BLOCK_ROWS: one lane takes 16 rows)
ARROW_WAVE_ROWS, ARROW_BLOCK_ROWS = 1024, 4096


class LpArrowCol(ctypes.Structure):
    """lp_arrow_col (include/logparser_amd.h): one column of lp_result_arrow"""
    _fields_ = [("path", ctypes.c_char_p), ("name", ctypes.c_char_p), ("form", ctypes.c_int32), ("kind", ctypes.c_int32)]


ARROW_OWNER_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p)


class LpArrowOwner(ctypes.Structure):
    """lp_arrow_owner: called once when the last exported array structure is released"""
    _fields_ = [("free_fn", ARROW_OWNER_FN), ("ctx", ctypes.c_void_p)]


def strings_from_dict(valid, index, dict_off, dict_chars):
    """The rows of a dictionary-encoded STRING column (lp_result_table_dict) as
    a list of str | None: row k is dictionary entry index[k] --
    dict_chars[dict_off[j], dict_off[j + 1]) (UTF-8) -- or None where valid[k]
    is 0."""
    chars = bytes(bytearray(dict_chars))
    off = [int(x) for x in dict_off]
    entries = [chars[off[j]:off[j + 1]].decode("utf-8") for j in range(len(off) - 1)]
    return [entries[int(i)] if v else None for v, i in zip(valid, index)]


MAP_ARRAYS = ("valid", "entry_off", "key_off", "key_chars", "val_off", "val_chars")


def maps_from_arrow(valid, entry_off, key_off, key_chars, val_off, val_chars):
    """The rows of an Arrow map<string,string> column (lp_result_table_map) as
    Python values: a dict per valid row, in the column's entry order, None for
    a row that is not valid.  Row k's entries are [entry_off[k], entry_off[k +
    1]); entry e's key is key_chars[key_off[e], key_off[e + 1]), its value
    val_chars[val_off[e], val_off[e + 1]) (UTF-8)."""
    kc, vc = bytes(bytearray(key_chars)), bytes(bytearray(val_chars))
    eo, ko, vo = ([int(x) for x in a] for a in (entry_off, key_off, val_off))
    out = []
    for k in range(len(eo) - 1):
        if not valid[k]:
            out.append(None)
            continue
        out.append({kc[ko[e]:ko[e + 1]].decode("utf-8"): vc[vo[e]:vo[e + 1]].decode("utf-8")
                    for e in range(eo[k], eo[k + 1])})
    return out


class LpResult(ctypes.Structure):
    """lp_result (include/logparser_amd.h): the SoA results of one batch"""
    _fields_ = [("n_lines", ctypes.c_int64), ("first_line", ctypes.c_int64), ("input_bytes", ctypes.c_uint64),
                ("input", ctypes.c_void_p),
                ("line_off", ctypes.c_void_p), ("columns", ctypes.c_void_p), ("columns_bytes", ctypes.c_uint64),
                ("arena", ctypes.c_void_p), ("arena_bytes", ctypes.c_uint64), ("shard_cap", ctypes.c_uint64),
                ("shard_off", ctypes.c_uint64 * ARENA_SHARDS), ("n_columns", ctypes.c_int32),
                ("on_host", ctypes.c_int32), ("column", ctypes.POINTER(LpColumn))]


class DissectionFailure(Exception):
    """nl.basjes.parse.core.exceptions.DissectionFailure"""


class FallbackRequired(Exception):
    """The device could not prove the line; hand it to the reference parser."""


class MissingDissectorsException(Exception):
    """nl.basjes.parse.core.exceptions.MissingDissectorsException"""


class InvalidDissectorException(Exception):
    """nl.basjes.parse.core.exceptions.InvalidDissectorException"""


class EngineUnavailable(RuntimeError):
    """The HIP library or a GPU is missing."""


# What a table call's code other than LP_OK raises, per family: code -> (exception, message);
# None: every other code (its message takes the code)
_SELECT_ERRORS = {None: (ValueError, "lp_result_select failed: %d")}
_WHERE_ERRORS = {LP_E_UNSUPPORTED: (FallbackRequired, "a term's values are derived on the host only: use select_where_from"),
                 LP_E_MISSING: (MissingDissectorsException, "lp_result_select_where: a path the parser does not deliver"),
                 None: (ValueError, "lp_result_select_where failed: %d")}
_TABLE_FROM_ERRORS = {None: (ValueError, "lp_result_table failed: %d")}
_TABLE_DEVICE_ERRORS = {LP_E_UNSUPPORTED: (FallbackRequired, "a column's values are derived on the host only: use table_from"),
                        None: (ValueError, "lp_result_table (device) failed: %d")}
_DICT_ERRORS = {LP_E_UNSUPPORTED: (FallbackRequired, "a column's values are derived on the host only: use table_dict_from"),
                None: (ValueError, "lp_result_table_dict failed: %d")}
_ARROW_ERRORS = {LP_E_UNSUPPORTED: (FallbackRequired, "a column's values are derived on the host only: use to_arrow"),
                 LP_E_MISSING: (MissingDissectorsException, "lp_result_arrow: a path the parser does not deliver"),
                 None: (ValueError, "lp_result_arrow failed: %d")}
_GROUP_ERRORS = {LP_E_UNSUPPORTED: (FallbackRequired, "a key's or measure's values are derived on the host only: use group_from"),
                 LP_E_MISSING: (MissingDissectorsException, "lp_result_group: a path the parser does not deliver"),
                 None: (ValueError, "lp_result_group failed: %d")}
_MAP_ERRORS = {LP_E_UNSUPPORTED: (FallbackRequired, "a map column's members are derived on the host only: use table_map_from"),
               LP_E_MISSING: (MissingDissectorsException, "lp_result_table_map: a path the parser does not deliver"),
               None: (ValueError, "lp_result_table_map failed: %d")}


def _sized_call(call, grow, errors):
    """The size protocol of the table calls: call() with the buffers at hand;
    on LP_E_NOMEM grow() makes what the reported lengths ask for and call()
    runs once more.  Any code but LP_OK then raises what errors (above) names."""
    rc = call()
    if rc == LP_E_NOMEM:
        grow()
        rc = call()
    if rc != LP_OK:
        exc, msg = errors.get(rc) or errors[None]
        raise exc(msg % rc if rc not in errors else msg)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineUnavailable("logparser_amd: %s not built (run __graft_entry__.build())" % LIB_PATH)
    # One HIP runtime per process: torch ships its own libamdhip64.so.7.  If it
    # is loaded first, the engine binds to it (same SONAME) and device pointers
    # and streams are shared; loaded the other way round, two runtimes fight
    # over the device and torch sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    c_char_pp = ctypes.POINTER(ctypes.c_char_p)
    L.lp_compile.restype = ctypes.c_void_p
    L.lp_compile.argtypes = [ctypes.c_char_p, c_char_pp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                             ctypes.c_char_p, ctypes.c_size_t]
    L.lp_free.argtypes = [ctypes.c_void_p]
    L.lp_possible_paths.restype = ctypes.c_int64
    L.lp_possible_paths.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]
    L.lp_compile_remapped.restype = ctypes.c_void_p
    L.lp_compile_remapped.argtypes = [ctypes.c_char_p, c_char_pp, ctypes.c_int, ctypes.POINTER(LpRemap), ctypes.c_int,
                                      ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_size_t]
    L.lp_possible_paths_remapped.restype = ctypes.c_int64
    L.lp_possible_paths_remapped.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(LpRemap), ctypes.c_int,
                                             ctypes.c_char_p, ctypes.c_size_t]
    L.lp_compile_dissectors.restype = ctypes.c_void_p
    L.lp_compile_dissectors.argtypes = [ctypes.c_char_p, c_char_pp, ctypes.c_int, ctypes.POINTER(LpRemap), ctypes.c_int,
                                        ctypes.POINTER(LpDissector), ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_size_t]
    L.lp_possible_paths_dissectors.restype = ctypes.c_int64
    L.lp_possible_paths_dissectors.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(LpRemap), ctypes.c_int,
                                               ctypes.POINTER(LpDissector), ctypes.c_int, ctypes.c_char_p,
                                               ctypes.c_size_t]
    L.lp_parse_batch.restype = ctypes.c_int
    L.lp_parse_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p]
    L.lp_parse_batch_at.restype = ctypes.c_int
    L.lp_parse_batch_at.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int,
                                    ctypes.c_void_p]
    L.lp_sync.argtypes = [ctypes.c_void_p]
    L.lp_num_lines.restype = ctypes.c_int64
    L.lp_num_lines.argtypes = [ctypes.c_void_p]
    L.lp_line_status.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    L.lp_line_offset.restype = ctypes.c_int64
    L.lp_line_offset.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    L.lp_line_record_json.restype = ctypes.c_int64
    L.lp_line_record_json.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_char_p, ctypes.c_size_t]
    L.lp_counters.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.lp_last_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    L.lp_histograms.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    L.lp_last_bytes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    L.lp_set_option.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64]
    L.lp_reserve.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64]
    L.lp_result_view.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult)]
    L.lp_result_copy.restype = ctypes.c_int64
    L.lp_result_copy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                 ctypes.POINTER(LpResult)]
    L.lp_result_record_json.restype = ctypes.c_int64
    L.lp_result_record_json.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, ctypes.c_char_p,
                                        ctypes.c_size_t]
    L.lp_result_emit.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, EMIT_FN, ctypes.c_void_p]
    L.lp_result_table.restype = ctypes.c_int
    L.lp_result_table.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, ctypes.c_int64,
                                  ctypes.POINTER(LpTableCol), ctypes.c_int, ctypes.c_int]
    L.lp_result_table_map.restype = ctypes.c_int
    L.lp_result_table_map.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, ctypes.c_int64,
                                      ctypes.POINTER(LpTableMapCol), ctypes.c_int, ctypes.c_int]
    L.lp_result_select.restype = ctypes.c_int
    L.lp_result_select.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, ctypes.c_int64,
                                   ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.lp_result_select_where.restype = ctypes.c_int
    L.lp_result_select_where.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_uint32, ctypes.POINTER(LpWhereTerm), ctypes.c_int, ctypes.c_void_p,
                                         ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
    L.lp_result_table_rows.restype = ctypes.c_int
    L.lp_result_table_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.POINTER(LpTableCol), ctypes.c_int, ctypes.c_int]
    L.lp_result_table_map_rows.restype = ctypes.c_int
    L.lp_result_table_map_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.POINTER(LpTableMapCol), ctypes.c_int, ctypes.c_int]
    L.lp_result_table_dict.restype = ctypes.c_int
    L.lp_result_table_dict.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, ctypes.c_int64,
                                       ctypes.POINTER(LpTableDictCol), ctypes.c_int, ctypes.c_int]
    L.lp_result_table_dict_rows.restype = ctypes.c_int
    L.lp_result_table_dict_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_void_p, ctypes.c_int64,
                                            ctypes.POINTER(LpTableDictCol), ctypes.c_int, ctypes.c_int]
    L.lp_result_group.restype = ctypes.c_int
    L.lp_result_group.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_int64, ctypes.c_int64,
                                  ctypes.POINTER(LpGroupKey), ctypes.c_int, ctypes.POINTER(LpGroupAgg), ctypes.c_int,
                                  ctypes.POINTER(LpGroupOut), ctypes.c_int]
    L.lp_result_group_rows.restype = ctypes.c_int
    L.lp_result_group_rows.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.POINTER(LpGroupKey), ctypes.c_int, ctypes.POINTER(LpGroupAgg), ctypes.c_int,
                                       ctypes.POINTER(LpGroupOut), ctypes.c_int]
    L.lp_result_arrow.restype = ctypes.c_int
    L.lp_result_arrow.argtypes = [ctypes.c_void_p, ctypes.POINTER(LpResult), ctypes.c_void_p, ctypes.c_int64,
                                  ctypes.c_int64, ctypes.POINTER(LpArrowCol), ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(ArrowSchema), ctypes.POINTER(ArrowDeviceArray)]
    L.lp_arrow_from_tables.restype = ctypes.c_int
    L.lp_arrow_from_tables.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.POINTER(LpTableCol), c_char_pp, ctypes.c_int,
                                       ctypes.POINTER(LpTableDictCol), c_char_pp, ctypes.c_int,
                                       ctypes.POINTER(LpTableMapCol), c_char_pp, ctypes.c_int,
                                       ctypes.POINTER(LpArrowOwner), ctypes.POINTER(ArrowSchema),
                                       ctypes.POINTER(ArrowDeviceArray)]
    L.lp_arrow_to_host.restype = ctypes.c_int
    L.lp_arrow_to_host.argtypes = [ctypes.POINTER(ArrowSchema), ctypes.POINTER(ArrowDeviceArray),
                                   ctypes.POINTER(ArrowArray)]
    L.lp_casts.restype = ctypes.c_int
    L.lp_casts.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.lp_describe.restype = ctypes.c_int64
    L.lp_describe.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.lp_synth_combined.restype = ctypes.c_int64
    L.lp_synth_combined.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_int64)]
    L.lp_synth.restype = ctypes.c_int64
    L.lp_synth.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
                           ctypes.c_size_t, ctypes.POINTER(ctypes.c_int64)]
    _lib = L
    return L


class LpRemap(ctypes.Structure):
    """lp_remap: Parser.addTypeRemapping(input, type, casts)"""
    _fields_ = [("input", ctypes.c_char_p), ("type", ctypes.c_char_p), ("casts", ctypes.c_int32)]


def _remap_array(remaps):
    """[(input, TYPE, casts)] -> (lp_remap array, count)"""
    arr = (LpRemap * max(1, len(remaps)))()
    for i, (n, t, c) in enumerate(remaps):
        arr[i] = LpRemap(n.encode(), t.encode(), c)
    return arr, len(remaps)


class LpDissector(ctypes.Structure):
    """lp_dissector: Parser.addDissector of a registrable dissector, by class name, with its settings"""
    _fields_ = [("name", ctypes.c_char_p), ("settings", ctypes.c_char_p)]


def _dissector_array(dissectors):
    """[(name, settings) or name] -> (lp_dissector array, count)"""
    ds = [(d, "") if isinstance(d, str) else tuple(d) for d in dissectors]
    arr = (LpDissector * max(1, len(ds)))()
    for i, (n, st) in enumerate(ds):
        arr[i] = LpDissector(n.encode(), (st or "").encode())
    return arr, len(ds)


def get_possible_paths(logformat, max_depth=15, remaps=(), dissectors=()):
    """Parser.getPossiblePaths(maxDepth) for a HttpdLoglineParser on logformat
    (remaps: [(input, TYPE, casts)], its type remappings; dissectors: [(class
    name, settings) or class name], its added dissectors)."""
    cap = 1 << 20
    out = ctypes.create_string_buffer(cap)
    arr, n_rm = _remap_array(list(remaps))
    dz, n_dz = _dissector_array(list(dissectors))
    n = lib().lp_possible_paths_dissectors(logformat.encode(), max_depth, arr, n_rm, dz, n_dz, out, cap)
    if n == LP_E_INVALID:  # (cap > 0 and an empty list is length 0, never -1: the arguments were refused)
        names = [bytes(dz[k].name).decode() for k in range(n_dz)]
        raise InvalidDissectorException("unknown dissector class, or a GeoIP database that cannot be read, among %r" % names if names
                                        else "lp_possible_paths_dissectors: invalid arguments")
    if n < 0:
        raise InvalidDissectorException("possible paths overflow")
    return [p for p in out.value.decode().split("\n") if p]


def synth_combined(seed, first_line, n_lines):
    """Deterministic synthetic 'combined' lines (BASELINE config 2 shape) as bytes."""
    cap = n_lines * 700 + 1024
    buf = ctypes.create_string_buffer(cap)
    got = ctypes.c_int64(0)
    nb = lib().lp_synth_combined(seed, first_line, n_lines, buf, cap, ctypes.byref(got))
    return buf.raw[:nb]


SYNTH_COMBINED, SYNTH_STRFTIME, SYNTH_NGINX, SYNTH_MIXED = 2, 3, 4, 5

# the LogFormat of each synthetic workload (BASELINE.json configs 2-5)
SYNTH_FORMATS = {
    SYNTH_COMBINED: "combined",
    SYNTH_STRFTIME: '%h %l %u [%{%d/%b/%Y %T}t.%{msec_frac}t] "%r" %>s %b "%{Referer}i" "%{User-Agent}i" %I %O',
    SYNTH_NGINX: '$remote_addr - $remote_user [$time_local] "$request" $status $body_bytes_sent "$http_referer" '
                 '"$http_user_agent" "$http_x_forwarded_for" $request_time $upstream_response_time $pipe',
}
# config 5: the three formats of the mixed corpus, one LogFormat per line, in
# HttpdLogFormatDissector's list order (hp/HttpdLogFormatDissector.java:110-125)
SYNTH_FORMATS[SYNTH_MIXED] = "\n".join((SYNTH_FORMATS[SYNTH_COMBINED], SYNTH_FORMATS[SYNTH_NGINX], "common"))


def synth(workload, seed, first_line, n_lines):
    """Deterministic synthetic lines of a BASELINE.json workload (SYNTH_*) as bytes."""
    cap = n_lines * 800 + 1024
    buf = ctypes.create_string_buffer(cap)
    got = ctypes.c_int64(0)
    nb = lib().lp_synth(workload, seed, first_line, n_lines, buf, cap, ctypes.byref(got))
    if nb < 0:
        raise ValueError("unknown synthetic workload %r" % workload)
    return buf.raw[:nb]


class ArrowExport:
    """One exported record batch (lp_result_arrow / lp_arrow_from_tables):
    .schema (ArrowSchema) and .device_array (ArrowDeviceArray), the ctypes
    structures a consumer of the Arrow C (Device) Data Interface takes by
    address.  The batch lives until release() (or until a consumer that moved
    the structures out releases them): it does not depend on the parser's next
    batch or on the parser."""

    def __init__(self, schema, device_array):
        self.schema, self.device_array = schema, device_array
        self._pa_schema = None

    @property
    def on_device(self):
        return self.device_array.device_type != ARROW_DEVICE_CPU

    def to_host_array(self):
        """lp_arrow_to_host itself: the ArrowArray of a deep host copy (every
        buffer byte for byte), the caller's to release; the export stays as it is."""
        tmp = None
        schema = self.schema
        if self._pa_schema is not None:  # (to_host moved .schema into pyarrow: export that one)
            schema = tmp = ArrowSchema()
            self._pa_schema._export_to_c(ctypes.addressof(tmp))
        out = ArrowArray()
        try:
            rc = lib().lp_arrow_to_host(ctypes.byref(schema), ctypes.byref(self.device_array), ctypes.byref(out))
        finally:
            if tmp is not None:
                tmp.release(ctypes.byref(tmp))
        if rc != LP_OK:
            raise ValueError("lp_arrow_to_host failed: %d" % rc)
        return out

    def to_host(self):
        """A pyarrow.RecordBatch of a deep host copy (lp_arrow_to_host); the
        export itself stays as it is and may be copied again.  (The first call
        moves .schema into a pyarrow.Schema, which later calls export again.)"""
        import pyarrow as pa
        out = self.to_host_array()
        if self._pa_schema is None:
            self._pa_schema = pa.Schema._import_from_c(ctypes.addressof(self.schema))
        return pa.RecordBatch._import_from_c(ctypes.addressof(out), self._pa_schema)

    def record_batch(self):
        """The pyarrow.RecordBatch of a HOST export, without a copy: pyarrow
        takes the structures over (this object is then released)."""
        import pyarrow as pa
        if self.on_device:
            raise ValueError("a device export: use to_host()")
        return pa.RecordBatch._import_from_c(ctypes.addressof(self.device_array.array), ctypes.addressof(self.schema))

    def release(self):
        """The release callbacks of whatever the consumer has not taken over"""
        a = self.device_array.array
        if a.release:
            a.release(ctypes.byref(a))
        if self.schema.release:
            self.schema.release(ctypes.byref(self.schema))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


_arrow_keep = {}  # owner context -> (what the exported buffers need alive, on_release)


def _arrow_owner_release(ctx):
    _, on_release = _arrow_keep.pop(ctx, (None, None))
    if on_release is not None:
        on_release()


_arrow_owner_cb = ARROW_OWNER_FN(_arrow_owner_release)
_arrow_next = [1]


def _ptr(a):
    """address of a numpy array / torch tensor (None: 0)"""
    if a is None:
        return None
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def arrow_from_tables(n_rows, plain=(), dicts=(), maps=(), device=-1, stream=None, on_release=None):
    """lp_arrow_from_tables: wrap columns that already stand in numpy arrays
    (device -1) or torch tensors of a device (device >= 0) into an ArrowExport
    without copying a value buffer.
      plain: [(name, str | int | float, valid, data[, path])] -- data the values
             array, for str the pair (offsets int64 [n_rows + 1], chars uint8);
             path (default: the name) "@line" makes the column large_binary;
      dicts: [(name, valid, index int32, dict_off int64, dict_chars uint8)];
      maps:  [(name, {MAP_ARRAYS name: array})] (an "entries_len" item overrides
             len(key_off) - 1).
    Children: the plain columns, the dictionary columns, the maps.  The arrays
    are kept alive until the consumer has released the batch's last array
    structure; on_release() is then called, once.  Raises ValueError(code)."""
    kinds = {str: CAST_STRING, int: CAST_LONG, float: CAST_DOUBLE}
    size = lambda a: int(a.numel()) if hasattr(a, "numel") else int(a.size)
    names = lambda items: (ctypes.c_char_p * max(1, len(items)))(*[it[0].encode() for it in items])
    P = (LpTableCol * max(1, len(plain)))()
    for k, it in enumerate(plain):
        name, typ, valid, data = it[:4]
        c = P[k]
        c.path = (it[4] if len(it) > 4 else name).encode()
        c.kind = kinds[typ]
        c.valid = _ptr(valid)
        if typ is str:
            c.i64, c.chars = _ptr(data[0]), _ptr(data[1])
            c.chars_cap = c.chars_len = size(data[1])
        elif typ is int:
            c.i64 = _ptr(data)
        else:
            c.f64 = _ptr(data)
    D = (LpTableDictCol * max(1, len(dicts)))()
    for k, (name, valid, index, doff, dchars) in enumerate(dicts):
        c = D[k]
        c.path = name.encode()
        c.valid, c.index, c.dict_off, c.dict_chars = _ptr(valid), _ptr(index), _ptr(doff), _ptr(dchars)
        c.dict_cap = c.dict_len = size(doff) - 1
        c.dict_chars_cap = c.dict_chars_len = size(dchars)
    M = (LpTableMapCol * max(1, len(maps)))()
    for k, (name, a) in enumerate(maps):
        c = M[k]
        c.path = name.encode()
        c.valid, c.entry_off = _ptr(a["valid"]), _ptr(a["entry_off"])
        c.key_off, c.val_off = _ptr(a["key_off"]), _ptr(a["val_off"])
        c.key_chars, c.val_chars = _ptr(a["key_chars"]), _ptr(a["val_chars"])
        c.entries_cap = c.entries_len = a.get("entries_len", size(a["key_off"]) - 1)
        c.key_chars_cap = c.key_chars_len = size(a["key_chars"])
        c.val_chars_cap = c.val_chars_len = size(a["val_chars"])
    ctx = _arrow_next[0]
    _arrow_next[0] += 1
    _arrow_keep[ctx] = ((list(plain), list(dicts), list(maps)), on_release)
    owner = LpArrowOwner(_arrow_owner_cb, ctx)
    schema, dev = ArrowSchema(), ArrowDeviceArray()
    rc = lib().lp_arrow_from_tables(device, ctypes.c_void_p(stream) if stream is not None else None, n_rows,
                                    P, names(plain), len(plain), D, names(dicts), len(dicts), M, names(maps), len(maps),
                                    ctypes.byref(owner), ctypes.byref(schema), ctypes.byref(dev))
    if rc != LP_OK:
        _arrow_keep.pop(ctx, None)  # (a failed call leaves the buffers the caller's: the owner is not called)
        err = ValueError("lp_arrow_from_tables failed: %d" % rc)
        err.code, err.schema, err.device_array = rc, schema, dev
        raise err
    return ArrowExport(schema, dev)


class BatchResult:
    """Results of one parse_batch call (valid until the parser's next batch)."""

    def __init__(self, parser):
        self._p = parser
        L = lib()
        rc = L.lp_sync(parser._h)
        if rc != LP_OK:
            raise EngineUnavailable("lp_sync failed: %d" % rc)
        self.n_lines = L.lp_num_lines(parser._h)
        st = np.zeros(max(1, self.n_lines), dtype=np.uint8)
        if self.n_lines:
            rc = L.lp_line_status(parser._h, 0, self.n_lines, st.ctypes.data)
            if rc != LP_OK:
                raise EngineUnavailable("lp_line_status failed: %d" % rc)
        self.status = st[: self.n_lines]
        c = (ctypes.c_uint64 * 13)()
        L.lp_counters(parser._h, c, 13)
        self.counters = {"lines": c[0], "ok": c[1], "bad": c[2], "fallback": c[3]}
        self.diag = {"overflow_waves": c[4], "retries": c[5], "arena_ovf": c[6], "uri_overflow_waves": c[7],
                     "deferred_chunks": c[8], "dfs_lines": c[9], "uri_repair_lines": c[10], "fixed_shape": c[11],
                     "walk_lines": c[12]}
        t = (ctypes.c_float * 3)()
        L.lp_last_timing(parser._h, t, 3)
        self.timing_ms = {"total": t[0], "index": t[1], "parse": t[2]}
        b = (ctypes.c_uint64 * 2)()
        L.lp_last_bytes(parser._h, b, 2)
        self.bytes_in, self.bytes_out = b[0], b[1]

    def record(self, i):
        """Values the reference Parser would deliver for line i (status OK)."""
        return json.loads(self.record_json(i))

    def record_json(self, i):
        cap = 1 << 16
        while True:
            out = ctypes.create_string_buffer(cap)
            n = lib().lp_line_record_json(self._p._h, i, out, cap)
            if n >= 0:
                return out.value.decode("utf-8")
            if n <= -100:
                cap = int(-n - 100) + 16
                continue
            if n == LP_E_STATE:
                raise ValueError("line %d has status %d" % (i, self.status[i]))
            raise EngineUnavailable("lp_line_record_json failed: %d" % n)

    def line_offset(self, i):
        return lib().lp_line_offset(self._p._h, i)

    def histograms(self):
        """lp_histograms into host memory: a dict view of the run counters"""
        return decode_histograms(self._p.histograms())

    def copy_to_host(self, with_input=True, buf=None):
        """lp_result_copy: every result of the batch in one host buffer (a
        numpy uint8 array, or buf when given and large enough); returns
        (buffer, LpResult)."""
        L = lib()
        need = -L.lp_result_copy(self._p._h, None, 0, 1 if with_input else 0, None)
        if need <= 0:
            raise EngineUnavailable("lp_result_copy failed: %d" % need)
        if buf is None or buf.nbytes < need:
            buf = np.empty(need, dtype=np.uint8)
        res = LpResult()
        rc = L.lp_result_copy(self._p._h, buf.ctypes.data, buf.nbytes, 1 if with_input else 0, ctypes.byref(res))
        if rc < 0:
            raise EngineUnavailable("lp_result_copy failed: %d" % rc)
        return buf, res

    def columns(self, res):
        """{(name, index): numpy view} of the columns of a host copy."""
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
        out = {}
        for k in range(res.n_columns):
            c = res.column[k]
            arr = np.ctypeslib.as_array((ctypes.c_uint8 * (c.elem_size * res.n_lines)).from_address(res.columns + c.offset))
            out[(c.name.decode(), c.index)] = arr.view(dt[c.elem_size])
        return out

    def emissions_from(self, res, i):
        """lp_result_emit: the Parsable.addDissection(base, type, name, value)
        calls delivering line i's values, from a host copy with the input;
        value = str | None | int."""
        out = []

        def cb(_ctx, base, typ, name, kind, p, n, l):
            v = None if kind == VALUE_NULL else l if kind == VALUE_LONG else ctypes.string_at(p, n).decode("utf-8")
            out.append((base.decode(), typ.decode(), name.decode(), v))

        fn = EMIT_FN(cb)
        rc = lib().lp_result_emit(self._p._h, ctypes.byref(res), i, fn, None)
        if rc < 0:
            raise ValueError("lp_result_emit(%d) failed: %d" % (i, rc))
        return out

    def _view(self):
        res = LpResult()
        rc = lib().lp_result_view(self._p._h, ctypes.byref(res))
        if rc != LP_OK:
            raise EngineUnavailable("lp_result_view failed: %d" % rc)
        return res

    @staticmethod
    def _rows_arg(rows, first, count, device):
        """(pointer, n_rows) of a row list: a contiguous int64 torch tensor on
        the device (device view) or numpy array (host copy); it excludes a window"""
        if first != 0 or count is not None:
            raise ValueError("rows excludes first / count")
        if device:
            if not (hasattr(rows, "data_ptr") and rows.is_cuda and str(rows.dtype) == "torch.int64" and rows.is_contiguous()):
                raise ValueError("rows: a contiguous int64 CUDA tensor expected")
            return rows.data_ptr(), int(rows.numel())
        if not (isinstance(rows, np.ndarray) and rows.dtype == np.int64 and rows.flags.c_contiguous and rows.ndim == 1):
            raise ValueError("rows: a contiguous int64 numpy array expected")
        return rows.ctypes.data, int(rows.size)

    def _window(self, rows, first, count, device):
        """(rows_p, first, count) of a table call: the window [first,
        first+count) (count None: up to the last line), or the row list"""
        if rows is not None:
            rows_p, n_rows = self._rows_arg(rows, first, count, device)
            return rows_p, 0, n_rows
        return None, first, self.n_lines - first if count is None else count

    def _entry(self, family, res, rows_p, first, count, cols, n_cols, threads):
        """the call of lp_result_<family> (rows_p None) or of lp_result_<family>_rows"""
        L, h = lib(), self._p._h
        if rows_p is None:
            fn = getattr(L, "lp_result_" + family)
            return lambda: fn(h, ctypes.byref(res), first, count, cols, n_cols, threads)
        fn = getattr(L, "lp_result_%s_rows" % family)
        return lambda: fn(h, ctypes.byref(res), rows_p, count, cols, n_cols, threads)

    def _timing(self, lo, hi):
        """lp_last_timing [lo, hi): HIP-event ms of the last device calls"""
        t = (ctypes.c_float * hi)()
        lib().lp_last_timing(self._p._h, t, hi)
        return t[lo:hi]

    def _select(self, res, mask, first, count, alloc, ptr):
        """lp_result_select with the table's size protocol: one call that
        reports the count, one that fills"""
        count = self.n_lines - first if count is None else count
        L = lib()
        n = ctypes.c_uint64(0)
        got = []  # the rows, once the count is known

        def call():
            return L.lp_result_select(self._p._h, ctypes.byref(res), first, count, mask, ptr(got[0]) if got else None,
                                      n.value if got else 0, ctypes.byref(n))
        _sized_call(call, lambda: got.append(alloc(int(n.value))), _SELECT_ERRORS)
        return got[0] if got else alloc(0)

    def select_device(self, mask, first=0, count=None):
        """lp_result_select on the device view: the lines of [first,
        first+count) whose status is in mask (SEL_* bits), ascending, as a
        torch int64 tensor of batch-relative line indices on the handle's
        device -- the rows= of table_device / table_map_device."""
        import torch
        dev = torch.device("cuda", self._p.device)
        return self._select(self._view(), mask, first, count, lambda n: torch.empty(n, dtype=torch.int64, device=dev),
                            lambda t: t.data_ptr())

    def select_from(self, res, mask, first=0, count=None):
        """lp_result_select from a host copy: a numpy int64 array"""
        return self._select(res, mask, first, count, lambda n: np.empty(n, dtype=np.int64), lambda a: a.ctypes.data)

    def select_timing(self):
        """HIP-event ms of the last device lp_result_select (both passes, the scan, the host's read of the count)"""
        return self._timing(11, 12)[0]

    def _select_where(self, res, terms, mask, first, count, alloc, ptr):
        """lp_result_select_where with the table's size protocol: one call
        that reports the count, one that fills"""
        arr, n_terms, keep = _where_array(terms)
        count = self.n_lines - first if count is None else count
        L = lib()
        n = ctypes.c_uint64(0)
        got = []  # the rows, once the count is known

        def call():
            return L.lp_result_select_where(self._p._h, ctypes.byref(res), first, count, mask, arr, n_terms,
                                            ptr(got[0]) if got else None, n.value if got else 0, ctypes.byref(n))
        _sized_call(call, lambda: got.append(alloc(int(n.value))), _WHERE_ERRORS)
        del keep
        return got[0] if got else alloc(0)

    def select_where_device(self, terms, mask=SEL_OK, first=0, count=None):
        """lp_result_select_where on the device view: the lines of [first,
        first+count) whose status is in mask and on whose table row the
        predicate of terms (a list of Where: AND over the groups of OR over a
        group's terms) holds, ascending, as a torch int64 tensor on the
        handle's device -- the rows= of table_device.  The predicate runs in
        one kernel over the parse columns; no column is built."""
        import torch
        dev = torch.device("cuda", self._p.device)
        return self._select_where(self._view(), terms, mask, first, count,
                                  lambda n: torch.empty(n, dtype=torch.int64, device=dev), lambda t: t.data_ptr())

    def select_where_from(self, res, terms, mask=SEL_OK, first=0, count=None):
        """lp_result_select_where from a host copy (with the input): a numpy int64 array, the same rows"""
        return self._select_where(res, terms, mask, first, count, lambda n: np.empty(n, dtype=np.int64),
                                  lambda a: a.ctypes.data)

    def select_where_timing(self):
        """HIP-event ms of the last device lp_result_select_where with terms: (the predicate kernel, the
        compaction: both passes, the scan, the host's read of the count)"""
        return tuple(self._timing(18, 20))

    def table_from(self, res, columns, first=0, count=None, threads=16, decode=True, rows=None):
        """lp_result_table: typed columns of rows [first, first+count) from a
        host copy -- or, with rows (a numpy int64 array of line indices, as
        select_from returns; not together with first / count), of exactly
        those lines (lp_result_table_rows).  columns: [(path, str | int |
        float)]; a path may be a pseudo-column (PSEUDO_COLUMNS).  Returns {path:
        (values, valid)}: values a list of str / None for STRING columns (bytes
        for "@line", whose text is not validated UTF-8; decode=False: the
        Arrow pair (offsets, chars bytes) as numpy arrays), a numpy int64 /
        float64 array for BIGINT / DOUBLE ones."""
        rows_p, first, count = self._window(rows, first, count, False)
        kinds = {str: CAST_STRING, int: CAST_LONG, float: CAST_DOUBLE}
        cols = (LpTableCol * len(columns))()
        keep = []
        for k, (path, typ) in enumerate(columns):
            c = cols[k]
            c.path = path.encode()
            c.kind = kinds[typ]
            valid = np.zeros(max(1, count), dtype=np.uint8)
            i64 = np.zeros(count + 1, dtype=np.int64)
            f64 = np.zeros(max(1, count), dtype=np.float64)
            c.valid, c.i64, c.f64 = valid.ctypes.data, i64.ctypes.data, f64.ctypes.data
            keep.append((valid, i64, f64))
        def grow():
            for k in range(len(columns)):
                if cols[k].kind == CAST_STRING:
                    buf = np.zeros(max(1, cols[k].chars_len), dtype=np.uint8)
                    keep[k] = keep[k] + (buf,)
                    cols[k].chars, cols[k].chars_cap = buf.ctypes.data, buf.nbytes
        _sized_call(self._entry("table", res, rows_p, first, count, cols, len(columns), threads), grow, _TABLE_FROM_ERRORS)
        out = {}
        for k, (path, typ) in enumerate(columns):
            valid, i64, f64 = keep[k][:3]
            ok = valid[:count].astype(bool)
            if typ is str and not decode:
                out[path] = ((i64, keep[k][3] if len(keep[k]) > 3 else np.zeros(0, np.uint8)), ok)
            elif typ is str:
                chars = keep[k][3].tobytes() if len(keep[k]) > 3 else b""
                text = (lambda b: b) if path == "@line" else (lambda b: b.decode("utf-8"))
                vals = [text(chars[i64[j]:i64[j + 1]]) if ok[j] else None for j in range(count)]
                out[path] = (vals, ok)
            else:
                out[path] = ((i64[:count] if typ is int else f64[:count]).copy(), ok)
        return out

    def table_buffers(self, columns, count=None, chars_cap=None, rows=None):
        """Device buffers for table_device(columns, buffers=...): per column
        [valid, i64 (STRING offsets / BIGINT values), f64 (DOUBLE), chars]
        (None where the kind has none); chars_cap: an int for every STRING
        column or {path: bytes}; rows: a row list (room for that many rows)."""
        import torch
        if rows is not None:
            if count is not None:
                raise ValueError("rows excludes first / count")
            count = int(rows.numel())
        count = self.n_lines if count is None else count
        dev = torch.device("cuda", self._p.device)
        keep = []
        for path, typ in columns:
            cap = chars_cap.get(path, 1) if isinstance(chars_cap, dict) else (chars_cap or 1)
            keep.append([torch.empty(max(1, count), dtype=torch.uint8, device=dev),
                         torch.empty(count + 1 if typ is str else max(1, count), dtype=torch.int64, device=dev)
                         if typ is not float else None,
                         torch.empty(max(1, count), dtype=torch.float64, device=dev) if typ is float else None,
                         torch.empty(max(1, cap), dtype=torch.uint8, device=dev) if typ is str else None])
        return keep

    def table_device(self, columns, first=0, count=None, chars_cap=None, buffers=None, rows=None):
        """lp_result_table on the device view: typed columns of rows [first,
        first+count) built in HBM -- or, with rows (a torch int64 tensor of
        line indices on the device, as select_device returns; not together
        with first / count), of exactly those lines (lp_result_table_rows).
        columns: [(path, str | int | float)].
        Returns {path: (values, valid)} of torch tensors on the handle's
        device: valid uint8 [count]; STRING columns the Arrow pair (offsets
        int64 [count + 1], chars uint8), BIGINT int64 / DOUBLE float64 [count].
        chars_cap: bytes allotted per STRING column (default: enough after a
        first call that reports the need); buffers: table_buffers(...) to
        fill instead of fresh ones."""
        rows_p, first, count = self._window(rows, first, count, True)
        kinds = {str: CAST_STRING, int: CAST_LONG, float: CAST_DOUBLE}
        res = self._view()
        cols = (LpTableCol * len(columns))()
        keep = buffers if buffers is not None else self.table_buffers(columns, count, chars_cap)
        for k, (path, typ) in enumerate(columns):
            c = cols[k]
            c.path = path.encode()
            c.kind = kinds[typ]
            valid, i64, f64, chars = keep[k]
            c.valid = valid.data_ptr()
            c.i64 = i64.data_ptr() if i64 is not None else 0
            c.f64 = f64.data_ptr() if f64 is not None else 0
            if chars is not None:
                c.chars = chars.data_ptr()
                c.chars_cap = chars.numel() if (chars_cap or buffers is not None) else 0
        def grow():
            import torch
            dev = torch.device("cuda", self._p.device)
            for k, (path, typ) in enumerate(columns):
                if typ is str and cols[k].chars_len > cols[k].chars_cap:
                    keep[k][3] = torch.empty(max(1, cols[k].chars_len), dtype=torch.uint8, device=dev)
                    cols[k].chars, cols[k].chars_cap = keep[k][3].data_ptr(), keep[k][3].numel()
        _sized_call(self._entry("table", res, rows_p, first, count, cols, len(columns), 0), grow, _TABLE_DEVICE_ERRORS)
        out = {}
        for k, (path, typ) in enumerate(columns):
            valid, i64, f64, chars = keep[k]
            if typ is str:
                out[path] = ((i64[:count + 1], chars[:cols[k].chars_len]), valid[:count])
            else:
                out[path] = ((i64 if typ is int else f64)[:count], valid[:count])
        return out

    def table_timing(self):
        """HIP-event ms of the last device lp_result_table's phases:
        {"values": k_table_values, "scans": offset scans, "chars": k_table_chars}"""
        return dict(zip(("values", "scans", "chars"), self._timing(5, 8)))

    def geoip_timing(self):
        """HIP-event ms of k_geoip_lines in the last batch (lp_last_timing [17]; 0 without a GeoIP stage)"""
        return self._timing(17, 18)[0]

    def _dict_call(self, res, paths, first, count, rows_p, threads, bufs, alloc, ptr):
        """lp_result_table_dict / _rows into bufs (per path [valid, index,
        dict_off, dict_chars]); after LP_E_NOMEM the dictionary's arrays are
        replaced by ones of the reported sizes and the call repeated once"""
        cols = (LpTableDictCol * len(paths))()
        for k, path in enumerate(paths):
            c = cols[k]
            c.path = path.encode()
            valid, index, doff, dchars = bufs[k]
            c.valid, c.index, c.dict_off, c.dict_chars = ptr(valid), ptr(index), ptr(doff), ptr(dchars)
            c.dict_cap, c.dict_chars_cap = len(doff) - 1, len(dchars)

        def grow():
            for k in range(len(paths)):
                c = cols[k]
                if c.dict_len > c.dict_cap:
                    bufs[k][2] = alloc(c.dict_len + 1, "int64")
                    c.dict_off, c.dict_cap = ptr(bufs[k][2]), c.dict_len
                if c.dict_chars_len > c.dict_chars_cap:
                    bufs[k][3] = alloc(max(1, c.dict_chars_len), "uint8")
                    c.dict_chars, c.dict_chars_cap = ptr(bufs[k][3]), len(bufs[k][3])
        _sized_call(self._entry("table_dict", res, rows_p, first, count, cols, len(paths), threads), grow, _DICT_ERRORS)
        return {path: (bufs[k][1][:count], (bufs[k][2][:cols[k].dict_len + 1], bufs[k][3][:cols[k].dict_chars_len]),
                       bufs[k][0][:count]) for k, path in enumerate(paths)}

    def table_dict_buffers(self, columns, count=None, dict_cap=None, dict_chars_cap=None, rows=None):
        """Device buffers for table_dict_device(columns, buffers=...): per
        path [valid uint8 [count], index int32 [count], dict_off int64
        [dict_cap + 1], dict_chars uint8 [dict_chars_cap]]; rows: a row list
        (room for that many rows)."""
        import torch
        if rows is not None:
            if count is not None:
                raise ValueError("rows excludes first / count")
            count = int(rows.numel())
        count = self.n_lines if count is None else count
        dev = torch.device("cuda", self._p.device)
        return [[torch.empty(max(1, count), dtype=torch.uint8, device=dev),
                 torch.empty(max(1, count), dtype=torch.int32, device=dev),
                 torch.empty((dict_cap or 0) + 1, dtype=torch.int64, device=dev),
                 torch.empty(max(1, dict_chars_cap or 0), dtype=torch.uint8, device=dev)] for _ in columns]

    def table_dict_device(self, columns, first=0, count=None, rows=None, buffers=None, dict_cap=None, dict_chars_cap=None):
        """lp_result_table_dict on the device view: dictionary-encoded STRING
        columns (Arrow dictionary<int32, utf8>) of rows [first, first+count)
        -- or, with rows (a torch int64 tensor on the device; not together
        with first / count), of exactly those lines -- built in HBM without
        writing the plain column's bytes.  columns: paths (any path
        table_device takes as str, "@line" included).  Returns {path: (index
        int32 [count], (dict_off int64 [dict_len + 1], dict_chars uint8),
        valid uint8 [count])} of torch tensors on the handle's device;
        entries in the order of first occurrence.  dict_cap / dict_chars_cap:
        room allotted per column (default: none, the call is repeated once
        with the sizes the first reports); buffers: table_dict_buffers(...)."""
        import torch
        rows_p, first, count = self._window(rows, first, count, True)
        dev = torch.device("cuda", self._p.device)
        dt = {"int64": torch.int64, "uint8": torch.uint8}
        bufs = buffers if buffers is not None else self.table_dict_buffers(columns, count, dict_cap, dict_chars_cap)
        return self._dict_call(self._view(), list(columns), first, count, rows_p, 0, bufs,
                               lambda n, t: torch.empty(n, dtype=dt[t], device=dev), lambda a: a.data_ptr())

    def table_dict_from(self, res, columns, first=0, count=None, threads=16, rows=None):
        """lp_result_table_dict from a host copy: the same arrays as
        table_dict_device, as numpy arrays (bit-identical to the device's)"""
        rows_p, first, count = self._window(rows, first, count, False)
        bufs = [[np.zeros(max(1, count), dtype=np.uint8), np.zeros(max(1, count), dtype=np.int32),
                 np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint8)] for _ in columns]
        for b in bufs:
            b[3] = b[3][:0]
        return self._dict_call(res, list(columns), first, count, rows_p, threads, bufs,
                               lambda n, t: np.zeros(n, dtype=t), lambda a: a.ctypes.data)

    def table_dict_timing(self):
        """HIP-event ms of the last device lp_result_table_dict's phases, summed over its columns:
        {"values": k_table_values of the rows, "insert": table reset + k_dict_insert,
        "index": k_dict_mark + rank scan + k_dict_index, "dict": the dictionary's values}"""
        return dict(zip(("values", "insert", "index", "dict"), self._timing(12, 16)))

    def _group(self, res, keys, aggs, first, count, rows_p, threads, alloc, ptr, groups_cap):
        """lp_result_group / _rows with the size protocol: a call that counts
        the groups (groups_cap: room allotted at once), one that fills"""
        karr, aarr = _group_args(keys, aggs)
        n_keys, n_aggs = len(karr) if karr else 0, len(aarr) if aarr else 0
        L, h = lib(), self._p._h
        out = LpGroupOut()
        group_of = alloc(max(1, count), "int32")
        out.group_of = ptr(group_of)
        bufs = {}

        def room(n):
            bufs["rep"] = alloc(max(1, n), "int64")
            bufs["aggs"] = [(alloc(max(1, n), "int64"), alloc(max(1, n), "uint8")) for _ in range(n_aggs)]
            out.rep, out.groups_cap = ptr(bufs["rep"]), n
            for j in range(n_aggs):
                aarr[j].value, aarr[j].valid = ptr(bufs["aggs"][j][0]), ptr(bufs["aggs"][j][1])

        room(groups_cap or 0)

        def call():
            if rows_p is None:
                return L.lp_result_group(h, ctypes.byref(res), first, count, karr, n_keys, aarr, n_aggs, ctypes.byref(out),
                                         threads)
            return L.lp_result_group_rows(h, ctypes.byref(res), rows_p, count, karr, n_keys, aarr, n_aggs,
                                          ctypes.byref(out), threads)
        _sized_call(call, lambda: room(out.n_groups), _GROUP_ERRORS)
        n = out.n_groups
        return {"n_groups": n, "rep": bufs["rep"][:n], "group_of": group_of[:count],
                "aggs": [(v[:n], ok[:n]) for v, ok in bufs["aggs"]]}

    def group_device(self, keys, aggs, first=0, count=None, rows=None, groups_cap=None):
        """lp_result_group on the device view: GROUP BY keys over rows [first,
        first+count) -- or, with rows (a torch int64 tensor on the device, as
        select_where_device returns; not together with first / count), over
        exactly those lines.  keys: [(path, str | int)] (at most 4; int: equal
        by value, str: by bytes; null is a key value of its own); aggs: a
        list of Agg (at most 8).  Returns {"n_groups", "rep": int64
        [n_groups] each group's first line, "group_of": int32 [count] every
        row's group, "aggs": [(value int64 [n_groups], valid uint8
        [n_groups])]} of torch tensors on the handle's device; groups in the
        order of first occurrence; table_device(keys, rows=rep) gives their
        key values.  No key or measure column is built.  groups_cap: room
        allotted at once (default: the call is repeated once the groups are
        counted)."""
        import torch
        rows_p, first, count = self._window(rows, first, count, True)
        dev = torch.device("cuda", self._p.device)
        dt = {"int64": torch.int64, "int32": torch.int32, "uint8": torch.uint8}
        return self._group(self._view(), keys, aggs, first, count, rows_p, 0,
                           lambda n, t: torch.empty(n, dtype=dt[t], device=dev), lambda a: a.data_ptr(), groups_cap)

    def group_from(self, res, keys, aggs, first=0, count=None, rows=None, threads=16, decode=True):
        """lp_result_group from a host copy (with the input): the same arrays
        as group_device, as numpy arrays (bit-identical to the device's).
        decode: also "keys": {path: (values, valid)}, the groups' key values
        as table_from(rows=rep) gives them."""
        rows_p, first, count = self._window(rows, first, count, False)
        out = self._group(res, keys, aggs, first, count, rows_p, threads, lambda n, t: np.zeros(n, dtype=t),
                          lambda a: a.ctypes.data, None)
        if decode:
            out["keys"] = self.table_from(res, list(keys), rows=np.ascontiguousarray(out["rep"]), threads=threads) if keys else {}
        return out

    def group_timing(self):
        """HIP-event ms of the last device lp_result_group's phases: {"insert": resets + k_group_insert,
        "index": k_dict_mark + rank scan + k_dict_index, "aggregate": fill + k_group_agg + k_group_finish}"""
        return dict(zip(("insert", "index", "aggregate"), self._timing(20, 23)))

    def _map_call(self, res, paths, first, count, threads, alloc, bufs, rows_p=None):
        """lp_result_table_map with lp_result_table's size protocol: a first
        call with the buffers at hand, a second after alloc() made the ones
        that were too small.  bufs: per path {name: array} (MAP_ARRAYS)."""
        ptr = (lambda a: a.data_ptr()) if hasattr(bufs[0]["valid"], "data_ptr") else (lambda a: a.ctypes.data)
        size = lambda a: int(a.numel()) if hasattr(a, "numel") else int(a.size)
        cols = (LpTableMapCol * len(paths))()

        def bind():
            for k, path in enumerate(paths):
                c, b = cols[k], bufs[k]
                c.path = path.encode()
                c.valid, c.entry_off = ptr(b["valid"]), ptr(b["entry_off"])
                c.key_off, c.val_off = ptr(b["key_off"]), ptr(b["val_off"])
                c.key_chars, c.val_chars = ptr(b["key_chars"]), ptr(b["val_chars"])
                c.entries_cap = min(size(b["key_off"]), size(b["val_off"])) - 1
                c.key_chars_cap, c.val_chars_cap = size(b["key_chars"]), size(b["val_chars"])
        bind()

        def grow():
            for k in range(len(paths)):
                c, b = cols[k], bufs[k]
                if c.entries_len > c.entries_cap:
                    b["key_off"], b["val_off"] = alloc(c.entries_len + 1, np.int64), alloc(c.entries_len + 1, np.int64)
                if c.key_chars_len > c.key_chars_cap:
                    b["key_chars"] = alloc(c.key_chars_len, np.uint8)
                if c.val_chars_len > c.val_chars_cap:
                    b["val_chars"] = alloc(c.val_chars_len, np.uint8)
            bind()
        _sized_call(self._entry("table_map", res, rows_p, first, count, cols, len(paths), threads), grow, _MAP_ERRORS)
        out = {}
        for k, path in enumerate(paths):
            c, b = cols[k], bufs[k]
            ne = int(c.entries_len)
            out[path] = {"valid": b["valid"][:count], "entry_off": b["entry_off"][:count + 1],
                         "key_off": b["key_off"][:ne + 1], "key_chars": b["key_chars"][:int(c.key_chars_len)],
                         "val_off": b["val_off"][:ne + 1], "val_chars": b["val_chars"][:int(c.val_chars_len)]}
        return out

    def table_map_from(self, res, paths, first=0, count=None, threads=16, decode=True, rows=None):
        """lp_result_table_map from a host copy: for each requested wildcard
        "TYPE:prefix.*" the Arrow map<string,string> column of rows [first,
        first+count) -- what ParsedRecord.getStringSet(name) / a Pig MAP
        column holds per record.  Returns {path: [dict | None per row]}, or
        with decode=False {path: {name: numpy array}} (MAP_ARRAYS).  rows (a
        numpy int64 array, not together with first / count): row k is line
        rows[k] (lp_result_table_map_rows)."""
        rows_p, first, count = self._window(rows, first, count, False)
        alloc = lambda n, dt: np.zeros(max(1, n), dtype=dt)
        bufs = [{"valid": alloc(count, np.uint8), "entry_off": alloc(count + 1, np.int64), "key_off": alloc(1, np.int64),
                 "val_off": alloc(1, np.int64), "key_chars": np.zeros(0, np.uint8), "val_chars": np.zeros(0, np.uint8)}
                for _ in paths]
        out = self._map_call(res, list(paths), first, count, threads, alloc, bufs, rows_p)
        if not decode:
            return out
        return {p: maps_from_arrow(*(a[n] for n in MAP_ARRAYS)) for p, a in out.items()}

    def table_map_buffers(self, paths, count=None, entries_cap=0, key_chars_cap=0, val_chars_cap=0):
        """Device buffers for table_map_device(paths, buffers=...): per path
        {name: torch tensor} (MAP_ARRAYS) with room for count rows, entries_cap
        entries and that many key / value bytes."""
        import torch
        count = self.n_lines if count is None else count
        dev = torch.device("cuda", self._p.device)
        mk = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
        return [{"valid": mk(max(1, count), torch.uint8), "entry_off": mk(count + 1, torch.int64),
                 "key_off": mk(entries_cap + 1, torch.int64), "val_off": mk(entries_cap + 1, torch.int64),
                 "key_chars": mk(key_chars_cap, torch.uint8), "val_chars": mk(val_chars_cap, torch.uint8)}
                for _ in paths]

    def table_map_device(self, paths, first=0, count=None, buffers=None, decode=True, rows=None):
        """lp_result_table_map on the device view: the map columns built in
        HBM.  buffers: table_map_buffers(...) to fill (a buffer that is too
        small is replaced in it) instead of fresh ones.  Returns what
        table_map_from returns; with decode=False the arrays are torch tensors
        on the handle's device.  FallbackRequired: the members are derived on
        the host only (table_map_from answers).  rows (a torch int64 tensor
        on the device, not together with first / count): row k is line
        rows[k] (lp_result_table_map_rows)."""
        import torch
        rows_p, first, count = self._window(rows, first, count, True)
        res = self._view()
        dev = torch.device("cuda", self._p.device)
        tdt = {np.int64: torch.int64, np.uint8: torch.uint8}
        alloc = lambda n, dt: torch.empty(max(1, n), dtype=tdt[dt], device=dev)
        bufs = buffers if buffers is not None else self.table_map_buffers(paths, count)
        out = self._map_call(res, list(paths), first, count, 0, alloc, bufs, rows_p)
        if not decode:
            return out
        return {p: maps_from_arrow(*(a[n].cpu().numpy() for n in MAP_ARRAYS)) for p, a in out.items()}

    def table_map_timing(self):
        """HIP-event ms of the last device lp_result_table_map, summed over
        its columns: {"count": k_map_count and the piece-base scan, "entries":
        k_map_entries and its scans, "fill": k_map_fill and k_map_chars}"""
        return dict(zip(("count", "entries", "fill"), self._timing(8, 11)))

    def arrow_call(self, res, columns, first=0, count=None, rows_p=None, threads=16):
        """lp_result_arrow itself: (code, ArrowSchema, ArrowDeviceArray).
        columns: [(path, str | int | float | "dict" | "map"[, field name])];
        rows_p: the address of a row list (then count is its length)."""
        kinds = {str: CAST_STRING, int: CAST_LONG, float: CAST_DOUBLE}
        cols = (LpArrowCol * max(1, len(columns)))()
        for k, col in enumerate(columns):
            path, typ = col[0], col[1]
            c = cols[k]
            c.path = path.encode()
            c.name = col[2].encode() if len(col) > 2 and col[2] is not None else None
            c.form = ARROW_DICT if typ == "dict" else ARROW_MAP if typ == "map" else ARROW_PLAIN
            c.kind = kinds.get(typ, 0)
        count = self.n_lines - first if count is None else count
        schema, dev = ArrowSchema(), ArrowDeviceArray()
        rc = lib().lp_result_arrow(self._p._h, ctypes.byref(res), rows_p, first, count, cols, len(columns), threads,
                                   ctypes.byref(schema), ctypes.byref(dev))
        return rc, schema, dev

    def _arrow(self, res, columns, first, count, rows, threads, device):
        rows_p, first, count = self._window(rows, first, count, device)
        rc, schema, dev = self.arrow_call(res, columns, first, count, rows_p, threads)
        if rc != LP_OK:
            exc, msg = _ARROW_ERRORS.get(rc) or _ARROW_ERRORS[None]
            raise exc(msg % rc if rc not in _ARROW_ERRORS else msg)
        return ArrowExport(schema, dev)

    def to_arrow(self, res, columns, first=0, count=None, rows=None, threads=16):
        """lp_result_arrow from a host copy: rows [first, first+count) -- or the
        lines of rows (a numpy int64 array) -- as a pyarrow.RecordBatch, imported
        through the Arrow C Data Interface without a further copy.  columns:
        [(path, str | int | float | "dict" | "map"[, field name])]: typed
        columns (pseudo-columns included; "@line" is large_binary),
        dictionary-encoded STRING columns, wildcard map columns."""
        import pyarrow  # noqa: F401  (ImportError here and nowhere else)
        return self._arrow(res, columns, first, count, rows, threads, False).record_batch()

    def to_arrow_device(self, columns, first=0, count=None, rows=None):
        """lp_result_arrow on the device view: an ArrowExport whose buffers are
        memory of the handle's device (ARROW_DEVICE_ROCM), bitmaps and int32 map
        offsets made on the GPU; rows: a torch int64 tensor on the device.  It
        outlives the parser's next batch and the parser: .to_host() a
        pyarrow.RecordBatch, .release() when done."""
        return self._arrow(self._view(), columns, first, count, rows, 0, True)

    def arrow_timing(self):
        """HIP-event ms of the last device lp_result_arrow's packaging kernels (lp_last_timing [16])"""
        return self._timing(16, 17)[0]

    def record_json_from(self, res, i):
        """lp_result_record_json: the record of line i from a host copy."""
        cap = 1 << 16
        while True:
            out = ctypes.create_string_buffer(cap)
            n = lib().lp_result_record_json(self._p._h, ctypes.byref(res), i, out, cap)
            if n >= 0:
                return out.value.decode("utf-8")
            if n <= -100:
                cap = int(-n - 100) + 16
                continue
            if n == LP_E_STATE:
                raise ValueError("line %d is not OK" % i)
            raise EngineUnavailable("lp_result_record_json failed: %d" % n)


class HttpdLoglineParser:
    """GPU-backed equivalent of new HttpdLoglineParser<>(RECORD.class, logformat)
    with addParseTarget(...) for each requested "TYPE:path"."""

    def __init__(self, logformat, fields=(), device=0, force_direct=False, reserve_lines=0, reserve_arena=0,
                 options=None):
        self.logformat = logformat
        self.fields = list(fields)
        self._targets = {}       # cleaned "TYPE:path" -> [Target] (Parser.targets)
        self._remaps = {}        # path -> {TYPE} (Parser.typeRemappings)
        self._remap_casts = {}   # "TYPE:path" -> casts of a remapped target
        self._dissectors = []    # (class name, settings) (Parser.addDissector)
        self._engine_fields = None
        self.device = device
        self.force_direct = force_direct
        self.reserve = (reserve_lines, reserve_arena)
        self.options = dict(options or {})  # lp_set_option(OPT_*, value) after lp_compile
        self._h = None
        self.device_program_ok = None
        self.unsupported_reason = ""

    # Parser.addParseTarget (core/Parser.java:517-635)
    def add_parse_target(self, *fields, setter=None, setter_policy=SetterPolicy.ALWAYS, value_class=str):
        """Request fields.  With a setter (a method name of the record passed
        to parse, or a callable taking (value) or (name, value)), parse(line,
        record) delivers them through it with Parser.store's rules: value_class
        str / int / float = a String / Long / Double setter, setter_policy a
        SetterPolicy."""
        self.fields.extend(fields)
        if setter is not None:
            for f in fields:
                self._targets.setdefault(cleanup_field_value(f), []).append(Target(setter, setter_policy, value_class))
        self._close()
        return self

    # Parser.addTypeRemapping(s) / setTypeRemappings (core/Parser.java:636-677)
    def add_type_remapping(self, input_name, new_type, casts=STRING_ONLY):
        name, typ = input_name.strip().lower(), new_type.strip().upper()
        if typ not in self._remaps.setdefault(name, set()):
            self._remaps[name].add(typ)
            self._remap_casts[typ + ":" + name] = casts
        self._close()
        return self

    # Parser.addDissector (core/Parser.java:154-160) of a dissector of the
    # reference's httpdlog-parser jar that is not there by default
    def add_dissector(self, name, settings=""):
        """Register a dissector by class name (simple, or fully qualified as
        Hive's "load:" / Pig's "-load:" give it) with its settings string.

        ScreenResolutionDissector: the settings are kept but, as in the
        reference, never reach the instance that dissects: a SCREENRESOLUTION
        is always split on "x".

        GeoIPCountryDissector / GeoIPCityDissector / GeoIPASNDissector /
        GeoIPISPDissector: the settings are the path of the MaxMind DB file,
        e.g. add_dissector("GeoIPCityDissector", "/path/to.mmdb").  Their
        outputs appear below every IP-typed path (country.name, city.name,
        location.latitude, asn.number, ...: get_possible_paths); a file that
        cannot be read as a database raises InvalidDissectorException when the
        parser is compiled.  A line whose address is a host name or a legacy
        form (anything but a dotted quad or RFC 4291 text) is FALLBACK."""
        self._dissectors.append((name, settings or ""))
        self._close()
        return self

    def add_type_remappings(self, mappings):
        for name, types in mappings.items():
            for t in types:
                self.add_type_remapping(name, t)
        return self

    def set_type_remappings(self, mappings):
        self._remaps, self._remap_casts = {}, {}
        return self.add_type_remappings(mappings or {})

    # Parser.getCasts (core/Parser.java:127-129)
    def get_casts(self, name):
        """CAST_* bits of a requested "TYPE:path" (None if unknown)"""
        name = cleanup_field_value(name)
        self._ensure()
        c = lib().lp_casts(self._h, name.encode())
        return None if c < 0 else c

    def _remap_list(self):
        """[(input, TYPE, casts)] in a stable order"""
        return [(n, t, self._remap_casts[t + ":" + n]) for n in sorted(self._remaps) for t in sorted(self._remaps[n])]

    def get_possible_paths(self, max_depth=15):
        return get_possible_paths(self.logformat, max_depth, self._remap_list(), self._dissectors)

    def _ensure(self):
        if self._h:
            return
        L = lib()
        fields = list(self.fields)
        self._engine_fields = fields
        arr = (ctypes.c_char_p * max(1, len(fields)))()
        for i, f in enumerate(fields):
            arr[i] = f.encode()
        rm, n_rm = _remap_array(self._remap_list())
        st = ctypes.c_int(0)
        err = ctypes.create_string_buffer(1024)
        dz, n_dz = _dissector_array(self._dissectors)
        h = L.lp_compile_dissectors(self.logformat.encode(), arr, len(fields), rm, n_rm, dz, n_dz, self.device,
                                    ctypes.byref(st), err, 1024)
        msg = err.value.decode(errors="replace")
        if not h:
            if st.value == LP_E_MISSING:
                raise MissingDissectorsException(msg)
            if st.value == LP_E_DEVICE:
                raise EngineUnavailable(msg)
            raise InvalidDissectorException(msg)
        self._h = h
        if self.force_direct:
            L.lp_set_option(h, OPT_FORCE_DIRECT, 1)
        if self.reserve[0] or self.reserve[1]:
            L.lp_reserve(h, self.reserve[0], self.reserve[1])
        for opt, val in self.options.items():
            if L.lp_set_option(h, opt, val) != LP_OK:
                raise ValueError("lp_set_option(%r, %r) rejected" % (opt, val))
        self.device_program_ok = st.value == LP_OK
        self.unsupported_reason = msg if st.value == LP_E_UNSUPPORTED else ""

    def parse_batch(self, data, stream=None):
        """Parse every '\\n'-separated line.  data: bytes / bytearray / numpy
        uint8 (host, copied to HBM) or a torch.uint8 CUDA tensor (in HBM)."""
        self._ensure()
        L = lib()
        s = ctypes.c_void_p(stream) if stream is not None else None
        if hasattr(data, "data_ptr") and getattr(data, "is_cuda", False):
            rc = L.lp_parse_batch(self._h, ctypes.c_void_p(data.data_ptr()), data.numel() * data.element_size(),
                                  BUF_DEVICE, s)
        else:
            if isinstance(data, np.ndarray):
                buf = np.ascontiguousarray(data, dtype=np.uint8)
                ptr, n = buf.ctypes.data, buf.nbytes
            else:
                buf = bytes(data)
                ptr, n = ctypes.cast(ctypes.c_char_p(buf), ctypes.c_void_p).value, len(buf)
            rc = L.lp_parse_batch(self._h, ctypes.c_void_p(ptr), n, BUF_HOST, s)
            L.lp_sync(self._h)  # the host buffer must outlive the copy
        if rc != LP_OK:
            raise EngineUnavailable("lp_parse_batch failed: %d" % rc)
        return BatchResult(self)

    def histograms(self, device_ptr=None):
        """lp_histograms of the last batch: the 1024 u64 words (numpy) in host
        memory, or written to device_ptr (a device buffer of 8 KiB on the
        handle's device, e.g. a torch tensor to all-reduce) when given"""
        self._ensure()
        if device_ptr is not None:
            rc = lib().lp_histograms(self._h, ctypes.c_void_p(device_ptr), 1)
            if rc != LP_OK:
                raise EngineUnavailable("lp_histograms failed: %d" % rc)
            return None
        out = np.zeros(HIST_WORDS, dtype=np.uint64)
        rc = lib().lp_histograms(self._h, out.ctypes.data, 0)
        if rc != LP_OK:
            raise EngineUnavailable("lp_histograms failed: %d" % rc)
        return out

    def run(self, data_ptr, nbytes, on_device=True, stream=None):
        """Lean batch call for benchmarks/pipelines: parse nbytes at data_ptr
        (a device pointer when on_device), wait, and return the device
        counters, HIP-event timings and algorithmic byte counts (no per-line
        copies to the host)."""
        self._ensure()
        L = lib()
        rc = L.lp_parse_batch(self._h, ctypes.c_void_p(data_ptr), nbytes, BUF_DEVICE if on_device else BUF_HOST,
                              ctypes.c_void_p(stream) if stream is not None else None)
        if rc != LP_OK:
            raise EngineUnavailable("lp_parse_batch failed: %d" % rc)
        rc = L.lp_sync(self._h)
        if rc != LP_OK:
            raise EngineUnavailable("lp_sync failed: %d" % rc)
        c = (ctypes.c_uint64 * 13)()
        L.lp_counters(self._h, c, 13)
        t = (ctypes.c_float * 5)()
        L.lp_last_timing(self._h, t, 5)
        b = (ctypes.c_uint64 * 4)()
        L.lp_last_bytes(self._h, b, 4)
        return {"lines": c[0], "ok": c[1], "bad": c[2], "fallback": c[3], "overflow_waves": c[4], "retries": c[5],
                "arena_ovf": c[6], "uri_overflow_waves": c[7], "deferred_chunks": c[8], "dfs_lines": c[9],
                "uri_repair_lines": c[10], "fixed_shape": c[11], "walk_lines": c[12],
                "ms_total": t[0], "ms_index": t[1], "ms_parse": t[2], "ms_parse_kernels": t[3], "ms_uri_kernels": t[4],
                "bytes_in": b[0], "bytes_out": b[1], "bytes_parse_kernels": b[2], "bytes_uri_kernels": b[3]}

    def parse(self, line, record=None):
        """Parser.parse(line) / parse(record, line) (core/Parser.java:700-756):
        without setters the record's values as {"TYPE:path": [values]}; with
        setters (add_parse_target(..., setter=...)) the values are delivered
        into `record` through them and `record` is returned.
        DissectionFailure for a bad line, FallbackRequired when the device
        cannot prove the line."""
        if isinstance(line, str):
            line = line.encode("utf-8")
        if b"\n" in line:
            raise ValueError("one line without terminator expected")
        r = self.parse_batch(line)
        if r.n_lines != 1:
            raise DissectionFailure("empty input")
        if r.status[0] == LINE_BAD:
            raise DissectionFailure("The input line does not match the specified log format.")
        if r.status[0] == LINE_FALLBACK:
            raise FallbackRequired(self.unsupported_reason or "line outside the device's proven subset")
        if not self._targets:
            return r.record(0)
        _, res = r.copy_to_host()
        return self.deliver(r.emissions_from(res, 0), record)

    def deliver(self, emissions, record):
        """Parser.store of one line's emissions (BatchResult.emissions_from)
        into `record` through the registered setters"""
        casts = {}

        def cast_of(name):
            if name not in casts:
                casts[name] = self.get_casts(name)
            return casts[name]
        return deliver(emissions, record, self._targets, cast_of, self._remaps)

    def describe(self):
        self._ensure()
        out = ctypes.create_string_buffer(1 << 16)
        lib().lp_describe(self._h, out, 1 << 16)
        return out.value.decode()

    def _close(self):
        if self._h:
            lib().lp_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self._close()
        except Exception:
            pass


# lp_histograms layout (include/logparser_amd.h)
HIST_WORDS = 1024
HIST_METHODS = ["GET", "POST", "HEAD", "PUT", "DELETE", "OPTIONS", "PATCH", "CONNECT", "TRACE", "PROPFIND", "MKCOL",
                "COPY", "MOVE", "LOCK", "UNLOCK", "(other)", "(none)"]


def decode_histograms(h):
    """the words of lp_histograms (or their all-reduced sum) as a dict"""
    h = [int(x) for x in h]
    return {
        "lines": h[0], "ok": h[1], "bad": h[2], "fallback": h[3],
        "token_null": h[16:32], "token_present": h[32:48],
        "status_other": h[48],
        "methods": {m: h[64 + i] for i, m in enumerate(HIST_METHODS) if h[64 + i]},
        "status": {c: h[100 + c] for c in range(100, 600) if h[100 + c]},
    }
