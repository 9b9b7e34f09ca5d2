"""The core of the grouped aggregates (csrc/lp_group.h over lp_dict.h) under
ASan + UBSan and under ThreadSanitizer: tests/emu/group_emu.cpp, a program
with its own main, run directly (nothing is loaded into Python).  It groups and
aggregates a corpus through the host build of the key hash, the insert's
same(r) rule, the accumulate / merge rules and the block-flush and wave-peel
shapes, from 1, 4 and 7 threads with whole and 1-bit hashes, against a
std::map built in row order."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
SRC = os.path.join(ROOT, "tests", "emu", "group_emu.cpp")
HDRS = [os.path.join(ROOT, "logparser_amd", "csrc", h) for h in ("lp_group.h", "lp_dict.h")]
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
TSAN = ["-fsanitize=thread", "-fno-omit-frame-pointer"]


def _build(name, flags):
    prog = os.path.join(BUILD, name)
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(prog) or os.path.getmtime(prog) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        tmp = "%s.%d.tmp" % (prog, os.getpid())  # renamed into place: parallel workers never see half a file
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-pthread", "-o", tmp] + flags + [SRC], check=True)
        os.replace(tmp, prog)
    return prog


def _run(prog):
    r = subprocess.run([prog], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "total: 0 differ" in r.stdout, r.stdout
    for bits in (0, 1):
        for threads in (1, 4, 7):
            assert "bits %d threads %d:" % (bits, threads) in r.stdout, r.stdout


def test_sanitized_standalone_program():
    _run(_build("group_emu_san", ASAN))


def test_thread_sanitized_standalone_program():
    _run(_build("group_emu_tsan", TSAN))
