"""The term rules of lp_result_select_where (csrc/lp_pred.h) under ASan +
UBSan: tests/emu/pred_emu.cpp, a program with its own main, run directly
(nothing is loaded into Python).  It checks each byte op against memcmp /
memmem / std::string and each LONG op against plain C++, with every value in a
heap block of exactly its aligned-word extent: an over-read is an ASan error."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")


def test_sanitized_standalone_program():
    src = os.path.join(ROOT, "tests", "emu", "pred_emu.cpp")
    hdrs = [os.path.join(ROOT, "logparser_amd", "csrc", h) for h in ("lp_pred.h", "lp_value.h")]
    prog = os.path.join(BUILD, "pred_emu_san")
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(prog) or os.path.getmtime(prog) < max(os.path.getmtime(p) for p in [src] + hdrs):
        tmp = "%s.%d.tmp" % (prog, os.getpid())
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", tmp, src], check=True)
        os.replace(tmp, prog)
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 500000
