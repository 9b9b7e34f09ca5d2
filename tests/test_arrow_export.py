"""Arrow C Data Interface export (lp_arrow_from_tables, lp_arrow_to_host), CPU
part: hand-built numpy columns through the host packaging (device -1), the raw
bitmaps against numpy.packbits, every batch imported and validated by pyarrow,
the schema's formats and flags, the ownership rules of the release callbacks,
and the stand-alone program of the host core (tests/emu/arrow_emu.cpp over
csrc/lp_arrow.h) under ASan + UBSan.  The GPU part is test_arrow_export_gpu.py."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pyarrow as pa  # noqa: F401  (the consumer that validates every batch)
import pytest

import arrow_corpus as ac
import logparser_amd as lpa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
EMU_SRC = os.path.join(ROOT, "tests", "emu", "arrow_emu.cpp")
CORE_HDR = os.path.join(ROOT, "logparser_amd", "csrc", "lp_arrow.h")
HEADER = os.path.join(ROOT, "include", "logparser_amd.h")
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def test_header_and_exports():
    """the header declares the three calls under the specification's guards, the library exports them"""
    from test_capi import declared_symbols
    assert {"lp_result_arrow", "lp_arrow_from_tables", "lp_arrow_to_host"} <= set(declared_symbols())
    L = lpa.lib()
    for s in ("lp_result_arrow", "lp_arrow_from_tables", "lp_arrow_to_host"):
        assert hasattr(L, s), s
    with open(HEADER) as f:
        src = f.read()
    for guard in ("#ifndef ARROW_C_DATA_INTERFACE", "#ifndef ARROW_C_DEVICE_DATA_INTERFACE", "#define ARROW_DEVICE_CPU 1",
                  "#define ARROW_DEVICE_ROCM 10", "#define ARROW_FLAG_NULLABLE 2"):
        assert guard in src, guard
    # without a handle / without columns: LP_E_INVALID, both outputs released
    schema, dev = lpa.ArrowSchema(), lpa.ArrowDeviceArray()
    col = lpa.LpArrowCol(b"@line", None, lpa.ARROW_PLAIN, lpa.CAST_STRING)
    res = lpa.LpResult()
    ctypes.memset(ctypes.byref(schema), 0xA5, ctypes.sizeof(schema))
    ctypes.memset(ctypes.byref(dev), 0xA5, ctypes.sizeof(dev))
    rc = L.lp_result_arrow(None, ctypes.byref(res), None, 0, 0, ctypes.byref(col), 1, 1, ctypes.byref(schema), ctypes.byref(dev))
    assert rc == lpa.LP_E_INVALID and ac.released(schema, dev)
    ctypes.memset(ctypes.byref(schema), 0xA5, ctypes.sizeof(schema))
    ctypes.memset(ctypes.byref(dev), 0xA5, ctypes.sizeof(dev))
    rc = L.lp_arrow_from_tables(-1, None, 0, None, None, 0, None, None, 0, None, None, 0, None, ctypes.byref(schema),
                                ctypes.byref(dev))
    assert rc == lpa.LP_E_INVALID and ac.released(schema, dev)  # n_cols == 0


def test_struct_layouts():
    """sizes and offsets of the ctypes mirrors equal the C structures' (a tiny C program prints them)"""
    structs = [("struct ArrowSchema", lpa.ArrowSchema), ("struct ArrowArray", lpa.ArrowArray),
               ("struct ArrowDeviceArray", lpa.ArrowDeviceArray), ("lp_arrow_col", lpa.LpArrowCol),
               ("lp_arrow_owner", lpa.LpArrowOwner)]
    os.makedirs(BUILD, exist_ok=True)
    prog = os.path.join(BUILD, "arrow_layout")
    csrc = prog + ".%d.c" % os.getpid()
    with open(csrc, "w") as f:
        f.write('#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n' % HEADER)
        for cname, cls in structs:
            for name, _ in cls._fields_:
                f.write('  printf("%%zu ", offsetof(%s, %s));\n' % (cname, name))
            f.write('  printf("%%zu\\n", sizeof(%s));\n' % cname)
        f.write('  return 0;\n}\n')
    tmp = "%s.%d.tmp" % (prog, os.getpid())
    subprocess.run(["gcc", "-std=c99", "-o", tmp, csrc], check=True)
    os.replace(tmp, prog)
    os.remove(csrc)
    out = subprocess.run([prog], capture_output=True, text=True, check=True).stdout.splitlines()
    for (cname, cls), line in zip(structs, out):
        want = [getattr(cls, name).offset for name, _ in cls._fields_] + [ctypes.sizeof(cls)]
        assert [int(x) for x in line.split()] == want, (cname, line, want)
    assert (ctypes.sizeof(lpa.ArrowSchema), ctypes.sizeof(lpa.ArrowArray), ctypes.sizeof(lpa.ArrowDeviceArray)) == (72, 80, 128)


def _check_bitmap(valid, n):
    """one LONG column of valid through the host packaging: the raw bitmap, the count, the import"""
    values = np.arange(n, dtype=np.int64)
    e = lpa.arrow_from_tables(n, plain=[("c", int, valid, values)])
    assert e.device_array.device_type == lpa.ARROW_DEVICE_CPU and e.device_array.device_id == -1
    assert not e.device_array.sync_event
    top = e.device_array.array
    assert top.length == n and top.null_count == 0 and top.offset == 0 and top.n_children == 1
    col = ac.child(top, 0)
    nulls = int((valid == 0).sum())
    assert col.length == n and col.null_count == nulls and col.offset == 0
    if nulls == 0:
        assert ac.buffer_ptr(col, 0) is None  # no nulls: no bitmap
    else:
        got = ac.host_bytes(col, 0, ac.bitmap_bytes(n))
        assert np.array_equal(got, ac.expected_bitmap(valid)), (n, np.flatnonzero(got != ac.expected_bitmap(valid))[:8])
    rb = e.record_batch()
    rb.validate(full=True)
    assert rb.column(0).to_pylist() == ac.plain_pylist(int, valid, values)


@pytest.mark.parametrize("n", ac.BITMAP_SIZES)
def test_bitmaps(n):
    """the bitmap equals numpy.packbits, every bit from n to the 64-byte multiple is 0, null_count is
    exact, a valid byte of 2 or 255 counts, all valid: a NULL pointer; then the same at byte skews 1..15"""
    for name in ac.PATTERNS:
        valid = ac.pattern(name, n)
        if n:
            assert set(np.unique(valid)) <= {0, 1, 2, 255}
        _check_bitmap(valid, n)
    for skew in range(1, 16):
        _check_bitmap(ac.skewed(ac.pattern("random", n, seed=skew), skew), n)
        _check_bitmap(ac.skewed(ac.pattern("last", n), skew), n)


def _all_forms(n):
    """numpy columns of every form, n rows, and the Python values of each"""
    rng = np.random.default_rng(n)
    words = [b"GET", b"POST", b"", "héllo".encode(), b"x" * 40]
    strs = [None if k % 4 == 1 else words[k % 5] for k in range(n)]
    lines = [b"\xff\xfe raw \x80" if k == 0 else b"line %d" % k for k in range(n)]
    dvals = [None if k % 5 == 2 else words[(k * 7) % 3] for k in range(n)]
    rows = []
    for k in range(n):
        if k % 6 == 3:
            rows.append(None)
        elif k % 6 == 4:
            rows.append([])
        elif k == 5:
            rows.append([(b"k%d" % j, b"v%d" % j) for j in range(300)])
        else:
            rows.append([(b"", b"empty key"), (b"a", b""), (b"b%d" % k, "ü".encode())])
    s_off, s_chars, s_valid = ac.string_col(strs)
    l_off, l_chars, l_valid = ac.string_col(lines)
    longs, l_ok = rng.integers(-2**62, 2**62, n), ac.pattern("third", n)
    dbls, d_ok = rng.random(n), ac.pattern("random", n)
    plain = [("BYTES:n", int, l_ok, longs), ("SECONDS:t", float, d_ok, dbls), ("STRING:s", str, s_valid, (s_off, s_chars)),
             ("raw", str, l_valid, (l_off, l_chars), "@line")]
    dicts = [("STRING:d",) + ac.dict_col(dvals)]
    maps = [("STRING:q.*", ac.map_col(rows))]
    want = {"BYTES:n": ac.plain_pylist(int, l_ok, longs), "SECONDS:t": ac.plain_pylist(float, d_ok, dbls),
            "STRING:s": ac.plain_pylist(str, s_valid, (s_off, s_chars)), "raw": lines,
            "STRING:d": lpa.strings_from_dict(*dicts[0][1:]), "STRING:q.*": ac.map_pylist(maps[0][1])}
    return plain, dicts, maps, want


@pytest.mark.parametrize("n", [0, 1, 6, 65, 1030])
def test_import_every_form(n):
    """every form in one batch: pyarrow validates it fully, its values are the Python decode of the
    same arrays, and a deep host copy (lp_arrow_to_host of a CPU batch) is an equal batch"""
    plain, dicts, maps, want = _all_forms(n)
    e = lpa.arrow_from_tables(n, plain=plain, dicts=dicts, maps=maps)
    copy = e.to_host()
    assert e.to_host().equals(copy)  # (the export stays as it is: copied again, also as a raw ArrowArray)
    raw = e.to_host_array()
    assert raw.length == n and raw.n_children == 6 and raw.release
    raw.release(ctypes.byref(raw))
    assert not raw.release
    e2 = lpa.arrow_from_tables(n, plain=plain, dicts=dicts, maps=maps)
    rb = e2.record_batch()
    for b in (rb, copy):
        b.validate(full=True)
        assert b.num_rows == n and b.schema.names == list(want)
        for name, vals in want.items():
            assert b.column(name).to_pylist() == vals, name
    assert rb.equals(copy)
    e.release()
    if n > 5:
        assert len(rb.column("STRING:q.*")[5].as_py()) == 300 and rb.column("STRING:q.*")[0].as_py()[0] == ("", "empty key")
        assert rb.column("raw")[0].as_py() == b"\xff\xfe raw \x80"  # invalid UTF-8 carried through large_binary


def test_schema_types_and_flags():
    """formats and flags exactly as the header's layout table"""
    plain, dicts, maps, _ = _all_forms(12)
    e = lpa.arrow_from_tables(12, plain=plain, dicts=dicts, maps=maps)
    s = e.schema
    N = lpa.ARROW_FLAG_NULLABLE
    assert s.format == b"+s" and s.flags == 0 and s.n_children == 6 and not s.metadata
    kids = [ac.child(s, k) for k in range(6)]
    assert [(k.format, k.flags, k.name) for k in kids] == [
        (b"l", N, b"BYTES:n"), (b"g", N, b"SECONDS:t"), (b"U", N, b"STRING:s"), (b"Z", N, b"raw"), (b"i", N, b"STRING:d"),
        (b"+m", N, b"STRING:q.*")]
    d = kids[4].dictionary.contents
    assert (d.format, d.flags, d.n_children) == (b"U", 0, 0)
    entries = ac.child(kids[5], 0)
    assert (entries.format, entries.flags, entries.name, entries.n_children) == (b"+s", 0, b"entries", 2)
    key, value = ac.child(entries, 0), ac.child(entries, 1)
    assert (key.format, key.flags, key.name) == (b"U", 0, b"key") and (value.format, value.flags, value.name) == (b"U", N, b"value")
    top = e.device_array.array
    m = ac.child(top, 5)
    ent = ac.child(m, 0)
    assert m.n_buffers == 2 and ent.n_buffers == 1 and ent.null_count == 0 and ac.buffer_ptr(ent, 0) is None
    assert ent.length == len(maps[0][1]["key_off"]) - 1
    val = ac.child(ent, 1)
    assert val.null_count == 0 and ac.buffer_ptr(val, 0) is None and val.n_buffers == 3
    # the map's second buffer: int32 offsets narrowed from entry_off
    off32 = ac.host_bytes(m, 1, 4 * 13).view(np.int32)
    assert np.array_equal(off32, maps[0][1]["entry_off"].astype(np.int32))
    # the STRING column's offsets and chars are the caller's arrays, not copies
    sc = ac.child(top, 2)
    assert ac.buffer_ptr(sc, 1) == plain[2][3][0].ctypes.data and ac.buffer_ptr(sc, 2) == plain[2][3][1].ctypes.data
    dc = ac.child(top, 4)
    assert dc.dictionary.contents.length == 3 and dc.dictionary.contents.null_count == 0
    rb = e.record_batch()
    assert [str(t) for t in rb.schema.types] == ["int64", "double", "large_string", "large_binary",
                                                 "dictionary<values=large_string, indices=int32, ordered=0>",
                                                 "map<large_string, large_string>"]
    assert not rb.schema.field("STRING:q.*").type.keys_sorted


def test_all_null_dictionary_with_empty_dictionary():
    n = 70
    valid, index = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    e = lpa.arrow_from_tables(n, dicts=[("d", valid, index, np.zeros(1, np.int64), np.zeros(0, np.uint8))])
    col = ac.child(e.device_array.array, 0)
    assert col.null_count == n and col.dictionary.contents.length == 0
    rb = e.record_batch()
    rb.validate(full=True)
    assert rb.column(0).to_pylist() == [None] * n and len(rb.column(0).dictionary) == 0


def test_map_with_too_many_entries_is_refused():
    """entries_len 2^31 (a faked length over tiny buffers: checked before anything is read):
    LP_E_INVALID, both outputs released, the owner not called"""
    m = ac.map_col([[(b"a", b"b")], None])
    m["entries_len"] = 2**31
    calls = []
    with pytest.raises(ValueError) as ei:
        lpa.arrow_from_tables(2, maps=[("q", m)], on_release=lambda: calls.append(1))
    assert ei.value.code == lpa.LP_E_INVALID and ac.released(ei.value.schema, ei.value.device_array) and not calls
    m["entries_len"] = 1
    lpa.arrow_from_tables(2, maps=[("q", m)]).record_batch().validate(full=True)


def _export(calls, n=40):
    plain, dicts, maps, _ = _all_forms(n)
    return lpa.arrow_from_tables(n, plain=plain, dicts=dicts, maps=maps, on_release=lambda: calls.append(1))


def _move_out(struct):
    """what a consumer does to take a structure over: copy it, mark the source released"""
    moved = type(struct).from_buffer_copy(struct)
    ctypes.memset(ctypes.byref(struct, type(struct).release.offset), 0, ctypes.sizeof(ctypes.c_void_p))
    assert not struct.release and moved.release
    return moved


def test_owner_called_once_after_the_last_array_release():
    # schema first, then the array
    calls = []
    e = _export(calls)
    e.schema.release(ctypes.byref(e.schema))
    assert not e.schema.release and calls == []
    a = e.device_array.array
    a.release(ctypes.byref(a))
    assert not a.release and calls == [1]
    # array first: the buffers go with it, the schema holds none
    calls = []
    e = _export(calls)
    a = e.device_array.array
    a.release(ctypes.byref(a))
    assert calls == [1] and e.schema.release
    e.schema.release(ctypes.byref(e.schema))
    assert calls == [1]
    e.release()  # (nothing left: no second call)
    assert calls == [1]
    # imported into pyarrow: the batch holds it, dropping the batch releases it
    calls = []
    rb = _export(calls).record_batch()
    gc.collect()
    assert calls == [] and rb.num_rows == 40
    del rb
    gc.collect()
    assert calls == [1]
    # a slice of one column keeps the buffers alive after the batch is gone
    calls = []
    rb = _export(calls).record_batch()
    col = rb.column("STRING:s")
    del rb
    gc.collect()
    assert calls == [] and col[0].as_py() == "GET"
    del col
    gc.collect()
    assert calls == [1]


def test_owner_with_children_moved_out():
    # a child moved out and released after its parent
    calls = []
    e = _export(calls)
    top = e.device_array.array
    kid = _move_out(ac.child(top, 2))
    top.release(ctypes.byref(top))
    assert calls == []
    e.schema.release(ctypes.byref(e.schema))
    assert calls == []
    kid.release(ctypes.byref(kid))
    assert not kid.release and calls == [1]
    # the dictionary column moved out: its dictionary is released through it
    calls = []
    e = _export(calls)
    top = e.device_array.array
    kid = _move_out(ac.child(top, 4))
    assert kid.dictionary.contents.release
    top.release(ctypes.byref(top))
    assert calls == []
    kid.release(ctypes.byref(kid))
    assert calls == [1]
    e.release()
    assert calls == [1]
    # the dictionary released through its parent, the batch
    calls = []
    e = _export(calls)
    e.release()
    assert calls == [1]
    # without an owner: nothing to call, nothing breaks
    plain, dicts, maps, _ = _all_forms(3)
    lpa.arrow_from_tables(3, plain=plain, dicts=dicts, maps=maps).release()


def test_last_timing_keeps_its_first_sixteen():
    """lp_last_timing [16] exists only for a caller that asks for 17 values (the header says so)"""
    with open(HEADER) as f:
        src = f.read()
    assert "[16] is\n * written only for n >= 17" in src


def _build(target, flags):
    os.makedirs(BUILD, exist_ok=True)
    if os.path.exists(target) and os.path.getmtime(target) >= max(os.path.getmtime(EMU_SRC), os.path.getmtime(CORE_HDR)):
        return target
    tmp = "%s.%d.tmp" % (target, os.getpid())  # renamed into place: parallel workers never see half a file
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-o", tmp] + flags + [EMU_SRC], check=True)
    os.replace(tmp, target)
    return target


def test_sanitized_standalone_program():
    """the host core under ASan + UBSan (leak check on), a program with its own main, run directly: the
    bit-packing against a per-bit loop for every n up to 1100 at every skew, batches of all forms
    built and released in every order with moved children, every buffer walked to its size"""
    prog = _build(os.path.join(BUILD, "arrow_emu_san"), ASAN)
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "total: 0 differ" in r.stdout and "bit-packing:" in r.stdout and "release orders:" in r.stdout, r.stdout
