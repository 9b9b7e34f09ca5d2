"""The MaxMind DB reader (csrc/lp_mmdb.h) and the GeoIP address parser / tree
walk (csrc/lp_geoip.h) under ASan + UBSan: tests/emu/mmdb_emu.cpp, a program
with its own main, run directly (nothing is loaded into Python).  It reads the
reference's four databases, the synthetic ones and several hundred damaged
copies of each, and parses every client value of the corpus."""
import os
import subprocess

import geoip_corpus as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
GOLD = os.path.join(ROOT, "tests", "golden", "geoip")


def test_sanitized_standalone_program(tmp_path):
    src = os.path.join(ROOT, "tests", "emu", "mmdb_emu.cpp")
    hdrs = [os.path.join(ROOT, "logparser_amd", "csrc", h) for h in ("lp_mmdb.h", "lp_geoip.h", "lp_program.h")]
    prog = os.path.join(BUILD, "mmdb_emu_san")
    os.makedirs(BUILD, exist_ok=True)
    if not os.path.exists(prog) or os.path.getmtime(prog) < max(os.path.getmtime(p) for p in [src] + hdrs):
        tmp = "%s.%d.tmp" % (prog, os.getpid())
        subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-o", tmp, src], check=True)
        os.replace(tmp, prog)
    values = sorted({h for h in gc.hosts() if "\n" not in h})
    assert len(values) > 300 and set(gc.UNDECIDED_HOSTS) <= set(values)
    vpath = tmp_path / "values.txt"
    vpath.write_text("".join(v + "\n" for v in values))
    dbs = [os.path.join(GOLD, f) for f in sorted(os.listdir(GOLD)) if f.endswith(".mmdb")]
    dbs += [gc.write_db(tmp_path, name)[0] for name in sorted(gc.CITY_DBS) + ["asn"]]
    assert len(dbs) == 9
    r = subprocess.run([prog, str(vpath)] + dbs, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    n_values, n_dbs, copies, still_valid = (int(x) for x in r.stdout.split()[1:5])
    assert n_values == len(values) and n_dbs == 9
    assert copies > 2000 and 0 < still_valid < copies
