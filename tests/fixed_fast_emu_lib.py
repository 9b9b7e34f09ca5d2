"""TEST-ONLY ctypes binding of tests/emu/fixed_fast_emu.cpp: the straight-line
first leaf of the fixed-shape instances (lp_device.h fixed_fast_leaf) on the
CPU against the generic matcher and the SIMPLE phase 1.  A library of its own
(tests/emu/_build/libfixed_fast_emu.so); never used by the product."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
LIB = os.path.join(BUILD, "libfixed_fast_emu.so")
SAN_MAIN = os.path.join(BUILD, "fixed_fast_emu_san")
PLAIN_MAIN = os.path.join(BUILD, "fixed_fast_emu_main")
CSRC = os.path.join(ROOT, "logparser_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "emu", "fixed_fast_emu.cpp"), os.path.join(CSRC, "plan.cpp")]
HDRS = [os.path.join(CSRC, h) for h in ("lp_device.h", "lp_fixed.h", "lp_program.h", "plan.h")]
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
STATS = ("views", "fast", "walked", "ok", "bad", "fallback", "redo", "offset_dependent")

_lib = None


def _stale(target):
    newest = max(os.path.getmtime(p) for p in SRCS + HDRS)
    return not os.path.exists(target) or os.path.getmtime(target) < newest


def _compile(target, flags):
    os.makedirs(BUILD, exist_ok=True)
    tmp = "%s.%d.tmp" % (target, os.getpid())  # renamed into place: parallel workers never see half a file
    subprocess.run(["g++", "-std=c++17", "-g", "-o", tmp] + flags + SRCS, check=True)
    os.replace(tmp, target)


def build_main(sanitized):
    """The stand-alone program (its own main), plain or under ASan + UBSan; run it directly."""
    target = SAN_MAIN if sanitized else PLAIN_MAIN
    if _stale(target):
        _compile(target, ["-O1", "-DFF_MAIN"] + (SAN_FLAGS if sanitized else []))
    return target


def lib():
    global _lib
    if _lib is None:
        if _stale(LIB):
            _compile(LIB, ["-O2", "-fPIC", "-shared"])
        L = ctypes.CDLL(LIB)
        L.ff_new.restype = ctypes.c_void_p
        L.ff_new.argtypes = [ctypes.c_char_p]
        L.ff_free.argtypes = [ctypes.c_void_p]
        L.ff_shape.argtypes = [ctypes.c_void_p]
        L.ff_run.restype = ctypes.c_int64
        L.ff_run.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64, ctypes.c_int,
                             ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
        _lib = L
    return _lib


def limits():
    """(head bytes, tail bytes, CLFNUMBER digits, %>s window bytes) of fixed_fast_leaf"""
    return tuple(lib().ff_limit(k) for k in range(4))


ALL_OFFSETS = -2
ROTATE = -1


class Fast:
    """"combined" or "common" with every path: its fixed-shape instance."""

    def __init__(self, name):
        self.h = lib().ff_new(name.encode())
        if not self.h:
            raise RuntimeError("%s is not a fixed shape" % name)

    def run(self, lines, off=ROTATE):
        """lines (bytes, no terminator) through the fast leaf, the instance's
        first leaf and phase 1 against the generic ones, each at window offset
        off (ROTATE: line i at i mod 64; ALL_OFFSETS: at all 64):
        (differing views, stats, per-line flags (1 fast, 2 walked), first difference)"""
        data = b"\n".join(lines) + b"\n"
        stats = (ctypes.c_int64 * 8)()
        flags = np.zeros(len(lines), dtype=np.uint8)
        first = ctypes.create_string_buffer(1024)
        n = lib().ff_run(self.h, data, len(data), off, stats, flags.ctypes.data, first, len(first))
        return n, dict(zip(STATS, stats)), flags, first.value.decode()

    def __del__(self):
        try:
            lib().ff_free(self.h)
        except Exception:
            pass
