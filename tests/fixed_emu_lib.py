"""TEST-ONLY ctypes binding of tests/emu/fixed_emu.cpp: the fixed-shape
instances of the parse kernel (lp_fixed.h) on the CPU -- the table against
plan.cpp's Program, the fixed matcher against the generic one, and the
adversarial line set the CPU and GPU tests share.  A library of its own
(tests/emu/_build/libfixed_emu.so); never used by the product."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
LIB = os.path.join(BUILD, "libfixed_emu.so")
SAN_MAIN = os.path.join(BUILD, "fixed_emu_san")
CSRC = os.path.join(ROOT, "logparser_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "emu", "fixed_emu.cpp"), os.path.join(CSRC, "plan.cpp")]
HDRS = [os.path.join(CSRC, h) for h in ("lp_device.h", "lp_fixed.h", "lp_program.h", "plan.h")]
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
SHAPES = {"combined": 1, "common": 2}

_lib = None


def _stale(target):
    newest = max(os.path.getmtime(p) for p in SRCS + HDRS)
    return not os.path.exists(target) or os.path.getmtime(target) < newest


def _compile(target, flags):
    os.makedirs(BUILD, exist_ok=True)
    tmp = "%s.%d.tmp" % (target, os.getpid())  # renamed into place: parallel workers never see half a file
    subprocess.run(["g++", "-std=c++17", "-g", "-o", tmp] + flags + SRCS, check=True)
    os.replace(tmp, target)


def build_sanitized_main():
    """The stand-alone program (its own main) under ASan + UBSan; run it directly."""
    if _stale(SAN_MAIN):
        _compile(SAN_MAIN, ["-O1", "-DFX_MAIN"] + SAN_FLAGS)
    return SAN_MAIN


def lib():
    global _lib
    if _lib is None:
        if _stale(LIB):
            _compile(LIB, ["-O2", "-fPIC", "-shared"])
        L = ctypes.CDLL(LIB)
        L.fx_new.restype = ctypes.c_void_p
        L.fx_new.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.fx_free.argtypes = [ctypes.c_void_p]
        L.fx_shape_of.argtypes = [ctypes.c_void_p]
        L.fx_table_diff.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.fx_diff.restype = ctypes.c_int64
        L.fx_diff.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int,
                              ctypes.POINTER(ctypes.c_int64), ctypes.c_char_p, ctypes.c_int]
        L.fx_adv_get.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        _lib = L
    return _lib


class Fixed:
    """The plan of a LogFormat (one per line of `logformat`) with `fields`."""

    def __init__(self, logformat, fields):
        arr = (ctypes.c_char_p * max(1, len(fields)))()
        for i, f in enumerate(fields):
            arr[i] = f.encode()
        err = ctypes.create_string_buffer(512)
        self.h = lib().fx_new(logformat.encode(), arr, len(fields), err, 512)
        if not self.h:
            raise RuntimeError("plan failed: %s" % err.value.decode())

    def shape(self):
        """lp_fixed.h fixed_shape_of: 0 none, 1 combined, 2 common"""
        return lib().fx_shape_of(self.h)

    def table_diff(self, shape):
        """fields of the compiled Program that differ from the shape's table"""
        out = ctypes.create_string_buffer(1 << 16)
        n = lib().fx_table_diff(self.h, shape, out, len(out))
        return n, out.value.decode()

    def diff(self, shape, data, off=-1):
        """Lines of data (bytes, '\\n'-separated) on which the fixed and the
        generic instance differ, each line at window offset off (-1: line i at
        i mod 64): (count, {status: lines}, first difference)"""
        stats = (ctypes.c_int64 * 5)()
        first = ctypes.create_string_buffer(1024)
        n = lib().fx_diff(self.h, shape, data, len(data), off, stats, first, len(first))
        return n, {"lines": stats[0], "ok": stats[1], "bad": stats[2], "fallback": stats[3], "redo": stats[4]}, \
            first.value.decode()

    def __del__(self):
        try:
            lib().fx_free(self.h)
        except Exception:
            pass


def adversarial(shape):
    """The adversarial lines (bytes, no terminator) built from the shape's valid line."""
    L = lib()
    buf = ctypes.create_string_buffer(16384)
    out = []
    for i in range(L.fx_adv_count(shape)):
        n = L.fx_adv_get(shape, i, buf, len(buf))
        assert n >= 0
        out.append(buf.raw[:n])
    return out
