"""TEST-ONLY ctypes binding of tests/emu/owner_emu.cpp: the owner lookup of
the URI kernels' cooperative passes (lp_owner.h) on the CPU, against its
definition.  A library of its own (tests/emu/_build/libowner_emu.so); never
used by the product."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
LIB = os.path.join(BUILD, "libowner_emu.so")
SAN_MAIN = os.path.join(BUILD, "owner_emu_san")
SRCS = [os.path.join(ROOT, "tests", "emu", "owner_emu.cpp")]
HDRS = [os.path.join(ROOT, "logparser_amd", "csrc", "lp_owner.h")]
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]

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
        _compile(SAN_MAIN, ["-O1", "-DOW_MAIN"] + SAN_FLAGS)
    return SAN_MAIN


def lib():
    global _lib
    if _lib is None:
        if _stale(LIB):
            _compile(LIB, ["-O2", "-fPIC", "-shared"])
        L = ctypes.CDLL(LIB)
        L.ow_group_name.restype = ctypes.c_char_p
        L.ow_group_name.argtypes = [ctypes.c_int]
        L.ow_run_group.restype = ctypes.c_int64
        L.ow_run_group.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_char_p, ctypes.c_int]
        L.ow_check.restype = ctypes.c_int64
        L.ow_check.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64), ctypes.c_char_p,
                               ctypes.c_int]
        _lib = L
    return _lib


def groups():
    """the names of the vector groups owner_emu.cpp builds"""
    L = lib()
    return [L.ow_group_name(i).decode() for i in range(L.ow_groups())]


def run_group(name):
    """(differences, {vectors, items, rounds, empty_rounds}, first difference)"""
    L = lib()
    stats = (ctypes.c_int64 * 4)()
    first = ctypes.create_string_buffer(2048)
    n = L.ow_run_group(groups().index(name), stats, first, len(first))
    return n, {"vectors": stats[0], "items": stats[1], "rounds": stats[2], "empty_rounds": stats[3]}, \
        first.value.decode()


def check(counts):
    """one vector of 64 per-lane counts: (differences, items, first difference)"""
    assert len(counts) == 64
    arr = (ctypes.c_uint32 * 64)(*counts)
    items = ctypes.c_int64(0)
    first = ctypes.create_string_buffer(2048)
    n = lib().ow_check(arr, ctypes.byref(items), first, len(first))
    return n, items.value, first.value.decode()
