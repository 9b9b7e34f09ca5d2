"""The chunk kernel's staging pass on the CPU: the 64-byte block core
(bcls::classify64p) against build_masks and a byte-by-byte reference, as a
stand-alone program (tests/emu/stage_block_emu.cpp) built plain and under
ASan + UBSan and run directly; and the corpora of stage_block_corpus.py,
whose planted positions are re-derived from their bytes, so that a corpus
that misses a position fails here and not on the device."""
import os
import subprocess

import pytest

import corpora
import logparser_amd as lpa
import stage_block_corpus as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "emu", "_build")
SRC = os.path.join(ROOT, "tests", "emu", "stage_block_emu.cpp")
HDRS = [os.path.join(ROOT, "logparser_amd", "csrc", h) for h in ("lp_device.h", "lp_program.h", "lp_fixed.h")]
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def _program(name, flags):
    target = os.path.join(BUILD, name)
    newest = max(os.path.getmtime(p) for p in [SRC] + HDRS)
    if not os.path.exists(target) or os.path.getmtime(target) < newest:
        os.makedirs(BUILD, exist_ok=True)
        tmp = "%s.%d.tmp" % (target, os.getpid())  # renamed into place: parallel workers never see half a file
        subprocess.run(["g++", "-std=c++17", "-g", "-o", tmp] + flags + [SRC], check=True)
        os.replace(tmp, target)
    return target


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_block_core_against_build_masks(build):
    """every byte value at each of the 64 positions (alone and among 'a'), 64 x
    '\\n', random blocks of the bytes the staging pass tells apart: plane words,
    lf, guard and other exactly equal"""
    if build == "plain":
        prog, n = _program("stage_block_emu", ["-O2"]), 200000
    else:  # its own main, run directly: no preloaded runtime
        prog, n = _program("stage_block_emu_san", ["-O1"] + SAN_FLAGS), 50000
    r = subprocess.run([prog, str(n)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "%d blocks checked, 0 differ" % (2 * 64 * 256 + 1 + n) in r.stdout


@pytest.fixture(scope="module")
def base():
    return lpa.synth_combined(20261023, 0, 400).split(b"\n")[:-1]


def _consistent(data):
    """the two independent restatements of the terminator rules agree"""
    lines = corpora.split_hadoop(data)
    starts = sb.line_starts(data)
    assert len(lines) == len(starts)
    term = sb.terminators(data)
    assert [s for s in starts[1:]] == [t + 1 for t in term][:len(starts) - 1]
    for s, l in zip(starts, lines):
        assert data[s:s + len(l)] == l
    return lines, starts, term


def test_corpus_residues(base):
    data = sb.residues(base)
    lines, starts, term = _consistent(data)
    assert len(lines) < 5000
    assert {s % 64 for s in starts} == set(range(64))
    assert {len(l) for l in lines} >= set(range(131))
    # a terminator in byte 63, the next line at byte 0 of the next block
    assert sum(1 for t in term if t % 64 == 63 and t + 1 in starts) >= 4
    # lines across, and starts next to, every 1 KiB and 4 KiB mark of the batch
    ends = [s + len(l) for s, l in zip(starts, lines)]
    for step in (1024, 4096):
        marks = range(step, len(data) - 200, step)
        assert len(marks) >= 3
        inside = sum(1 for m in marks if any(s < m <= e for s, e in zip(starts, ends)))
        assert inside == len(marks)


def test_corpus_dense_starts(base):
    data = sb.dense_starts(base)
    lines, starts, term = _consistent(data)
    assert len(lines) < 5000
    counts = sb.block_counts(data)
    assert set(counts) >= set(sb.DENSE_COUNTS), sorted(set(counts))
    for plane in range(7):  # every bit plane of the per-lane count, 64 itself included
        assert any(c >> plane & 1 for c in counts)
    assert 64 in counts and 32 in counts
    # 64 consecutive '\n' from byte 0 of a block, and from byte 37
    runs = [i for i in range(len(data) - 63) if data[i:i + 64] == b"\n" * 64 and (i == 0 or data[i - 1] != 0x0A)]
    assert {i % 64 for i in runs} >= {0, 37}, runs
    # more than 64 starts within CB_MIN bytes: every chunk geometry has a chunk with excess lines
    assert any(sum(counts[i:i + sb.CB_MIN // 64 - 1]) > 64 + 8 for i in range(len(counts)))


def test_corpus_crlf(base):
    data = sb.crlf(base)
    lines, starts, term = _consistent(data)
    crlf_at = {i % 64 for i in range(len(data) - 1) if data[i:i + 2] == b"\r\n"}
    lone_at = {i % 64 for i in range(len(data)) if data[i] == 0x0D and data[i + 1:i + 2] != b"\n"}
    assert crlf_at >= set(sb.CR_BYTES) and lone_at >= set(sb.CR_BYTES), (crlf_at, lone_at)
    assert b"\r\r" in data and data.endswith(b"\r") and not data.endswith(b"\n\r")
    assert len(lines) == len(starts) and starts[-1] + len(lines[-1]) + 1 == len(data)


def test_corpus_boundaries(base):
    """whatever multiple of 64 in [CB_MIN, CB_MAX] a chunk is, one of its
    boundaries has a '\\n' two before it, one just before it and one on it"""
    data = sb.boundaries(base)
    lines, starts, term = _consistent(data)
    assert len(lines) < 5000
    tset = set(term)
    for cb in range(sb.CB_MIN, sb.CB_MAX + 1, 64):
        bounds = range(cb, len(data), cb)
        for d in (-2, -1, 0):  # t_hi - 1 | t_lo = the chunk before's t_hi | the chunk's first byte
            assert any(c + d in tset and not ({c - 2, c - 1, c} - {c + d}) & tset for c in bounds), (cb, d)


def test_corpus_guard_and_mixed(base):
    data = sb.guard_lines(base)
    lines, _, _ = _consistent(data)
    assert sum(1 for l in lines if b"\t" in l) > 50 and sum(1 for l in lines if any(c >= 0x80 for c in l)) > 50
    data = sb.mixed(base, 3)
    lines, starts, term = _consistent(data)
    assert not data.endswith((b"\n", b"\r")) and lines[-1] == base[0]
    assert max(sb.block_counts(data)) == 64 and b"\r\n" in data
    assert any(sum(sb.block_counts(data)[i:i + 15]) > 72 for i in range(len(data) // 64))
