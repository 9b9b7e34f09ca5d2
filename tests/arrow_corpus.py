"""Inputs and references of the Arrow export tests (test_arrow_export.py on
hand-built numpy columns, test_arrow_export_gpu.py on the device's tables):
validity patterns and their bitmaps, numpy columns of every form, the Python
values pyarrow must show for them, and readers of the raw C structures."""
import ctypes

import numpy as np

import logparser_amd as lpa

# around every boundary of the bit-packing: a byte, the 16-row group of a lane, the
# 64-byte allocation unit (512 rows), the device kernel's wave (1024) and block (4096)
BITMAP_SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
PATTERNS = ("all", "none", "first", "last", "third", "random")


def bitmap_bytes(n):
    """bytes of a validity bitmap of n rows: a multiple of 64"""
    return ((n + 7) // 8 + 63) // 64 * 64


def pattern(name, n, seed=20261020):
    """valid bytes [n] of a named pattern; valid rows hold 1, 2 or 255"""
    rng = np.random.default_rng(seed + n)
    ok = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": np.arange(n) != 0,
          "last": np.arange(n) != n - 1, "third": np.arange(n) % 3 != 0, "random": rng.random(n) < 0.7}[name]
    return np.where(ok, rng.choice(np.array([1, 2, 255], np.uint8), n), 0).astype(np.uint8)


def expected_bitmap(valid):
    """Arrow's bitmap of valid bytes, padded with zero bits to the 64-byte multiple"""
    valid = np.asarray(valid)
    out = np.zeros(bitmap_bytes(len(valid)), np.uint8)
    bits = np.packbits(valid != 0, bitorder="little")
    out[:len(bits)] = bits
    return out


def skewed(a, skew):
    """a copy of uint8 array a that starts `skew` bytes past a 64-byte boundary"""
    buf = np.zeros(len(a) + 128, np.uint8)
    base = (-buf.ctypes.data) % 64 + skew
    view = buf[base:base + len(a)]
    view[:] = a
    assert len(a) == 0 or view.ctypes.data % 16 == skew % 16  # (numpy gives an empty view no address of its own)
    return view


def string_col(values):
    """(offsets int64, chars uint8, valid uint8) of bytes | None values"""
    off = np.zeros(len(values) + 1, np.int64)
    np.cumsum([len(v or b"") for v in values], out=off[1:])
    chars = np.frombuffer(b"".join(v or b"" for v in values), np.uint8).copy()
    return off, chars, np.array([v is not None for v in values], np.uint8)


def dict_col(values):
    """(valid, index int32, dict_off, dict_chars) of bytes | None values, entries by first occurrence"""
    seen, idx = {}, []
    for v in values:
        idx.append(0 if v is None else seen.setdefault(v, len(seen)))
    off, chars, _ = string_col(list(seen))
    return np.array([v is not None for v in values], np.uint8), np.array(idx, np.int32), off, chars


def map_col(rows):
    """{MAP_ARRAYS} of rows: a list of (key bytes, value bytes) pairs, or None"""
    entries = [kv for r in rows if r is not None for kv in r]
    eo = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r or ()) for r in rows], out=eo[1:])
    ko, kc, _ = string_col([k for k, _ in entries])
    vo, vc, _ = string_col([v for _, v in entries])
    return {"valid": np.array([r is not None for r in rows], np.uint8), "entry_off": eo, "key_off": ko, "key_chars": kc,
            "val_off": vo, "val_chars": vc}


def plain_pylist(typ, valid, data, binary=False):
    """what RecordBatch.to_pylist shows for a plain column"""
    if typ is str:
        off, chars = data
        raw = bytes(bytearray(chars))
        text = (lambda b: b) if binary else (lambda b: b.decode("utf-8"))
        return [text(raw[int(off[k]):int(off[k + 1])]) if valid[k] else None for k in range(len(valid))]
    return [typ(data[k]) if valid[k] else None for k in range(len(valid))]


def map_pylist(arrays):
    """... for a map column: a list of (key, value) pairs per valid row"""
    return [None if d is None else list(d.items()) for d in lpa.maps_from_arrow(*(arrays[n] for n in lpa.MAP_ARRAYS))]


def child(array, k):
    """child k of a ctypes ArrowArray / ArrowSchema"""
    assert 0 <= k < array.n_children
    return array.children[k].contents


def buffer_ptr(array, k):
    """buffer k of a ctypes ArrowArray as an address (None: a null pointer)"""
    assert 0 <= k < array.n_buffers
    return array.buffers[k]


def host_bytes(array, k, nbytes):
    """nbytes of buffer k of a HOST ArrowArray as a numpy uint8 array"""
    p = buffer_ptr(array, k)
    return np.frombuffer(ctypes.string_at(p, nbytes), np.uint8) if nbytes else np.zeros(0, np.uint8)


def released(schema, dev):
    """both outputs of a failed call are released"""
    return not schema.release and not dev.array.release
