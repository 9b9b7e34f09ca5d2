"""TEST-ONLY ctypes binding of tests/emu/geoip_emu.cpp: the CPU emulation with
the parser's added dissectors (dissectors_emu_lib.py) plus k_geoip_lines'
per-line work.  A library of its own; never used by the product or the
benchmark."""
import ctypes
import json
import os
import subprocess

from dissectors_emu_lib import CompileError, _cstrs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "emu", "_build", "libgeoip_emu.so")
SRCS = [os.path.join(ROOT, "tests", "emu", "geoip_emu.cpp"), os.path.join(ROOT, "logparser_amd", "csrc", "plan.cpp")]
DEPS = SRCS + [os.path.join(ROOT, "tests", "emu", f) for f in ("emu.cpp", "dissectors_emu.cpp")] + [
    os.path.join(ROOT, "logparser_amd", "csrc", h)
    for h in ("lp_device.h", "lp_program.h", "lp_value.h", "lp_table.h", "plan.h", "lp_geoip.h", "lp_mmdb.h")]

OK, BAD, FALLBACK = 0, 1, 2
LP_E_INVALID, LP_E_MISSING, LP_E_UNSUPPORTED = -1, -2, -3
MAX_VAL = 8
_lib = None


def build():
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= max(os.path.getmtime(p) for p in DEPS):
        return
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    tmp = "%s.%d.tmp" % (LIB, os.getpid())  # renamed into place: parallel workers never load half a library
    subprocess.run(["g++", "-std=c++17", "-g", "-O2", "-fPIC", "-shared", "-o", tmp] + SRCS, check=True)
    os.replace(tmp, LIB)


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(LIB)
        pp = ctypes.POINTER(ctypes.c_char_p)
        L.emu_new_dissectors.restype = ctypes.c_void_p
        L.emu_new_dissectors.argtypes = [ctypes.c_char_p, pp, ctypes.c_int, pp, pp, ctypes.c_int, pp, pp, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_int]
        L.emu_possible_paths_dissectors.restype = ctypes.c_int
        L.emu_possible_paths_dissectors.argtypes = [ctypes.c_char_p, ctypes.c_int, pp, pp, ctypes.c_int, pp, pp,
                                                    ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.emu_free.argtypes = [ctypes.c_void_p]
        L.emu_parse_in_geo.restype = ctypes.c_int
        L.emu_parse_in_geo.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_char_p,
                                       ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
        L.emu_casts.restype = ctypes.c_int
        L.emu_casts.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        _lib = L
    return _lib


class Emu:
    def __init__(self, logformat, fields, remaps=(), dissectors=()):
        """remaps: [(input path, new TYPE)]; dissectors: [(class name, settings)]"""
        self._keep = (_cstrs(fields), _cstrs([r[0] for r in remaps]), _cstrs([r[1] for r in remaps]),
                      _cstrs([d[0] for d in dissectors]), _cstrs([d[1] for d in dissectors]))
        st = ctypes.c_int(0)
        err = ctypes.create_string_buffer(1024)
        k = self._keep
        self.h = lib().emu_new_dissectors(logformat.encode(), k[0], len(fields), k[1], k[2], len(remaps), k[3], k[4],
                                          len(dissectors), ctypes.byref(st), err, 1024)
        self.status = st.value  # 0, or -3 with the planner's reason in err (every line FALLBACK)
        self.err = err.value.decode(errors="replace")
        if not self.h:
            raise CompileError(self.status, self.err)
        self.buf = ctypes.create_string_buffer(1 << 20)

    def parse_batch(self, data):
        """every '\\n'-terminated line of data parsed in place inside the whole
        buffer: [(status, record or None, the geo column's words)]"""
        n = len(data)
        buf = ctypes.create_string_buffer(data + b"\0" * 16, n + 16)
        rec = (ctypes.c_uint32 * MAX_VAL)()
        out, start = [], 0
        while start < n:
            end = data.find(b"\n", start)
            if end < 0:
                end = n
            st = lib().emu_parse_in_geo(self.h, ctypes.addressof(buf), start, end - start, self.buf, len(self.buf), rec)
            assert st in (0, 1, 2), (st, self.buf.value)
            out.append((st, json.loads(self.buf.value.decode("utf-8", errors="replace")) if st == 0 else None, list(rec)))
            start = end + 1
        return out

    def casts(self, target):
        c = lib().emu_casts(self.h, target.encode())
        return None if c < 0 else c

    def __del__(self):
        try:
            if self.h:
                lib().emu_free(self.h)
        except Exception:
            pass


def possible_paths(logformat, depth=15, remaps=(), dissectors=()):
    b = ctypes.create_string_buffer(1 << 20)
    n = lib().emu_possible_paths_dissectors(
        logformat.encode(), depth, _cstrs([r[0] for r in remaps]), _cstrs([r[1] for r in remaps]), len(remaps),
        _cstrs([d[0] for d in dissectors]), _cstrs([d[1] for d in dissectors]), len(dissectors), b, len(b))
    if n < 0:
        raise CompileError(n, "possible paths refused")
    return [p for p in b.value.decode().split("\n") if p]
