"""The fixed-shape instances of the parse kernel (lp_fixed.h) on the CPU: the
constant tables against what plan.cpp compiles, the host's predicate on
near-miss formats, and the fixed matcher / phase 1 against the generic ones
(tests/emu/fixed_emu.cpp), with and without mask planes."""
import subprocess

import pytest

import corpora
import fixed_emu_lib as fx
import logparser_amd as lpa

COMBINED = '%h %l %u %t "%r" %>s %b "%{Referer}i" "%{User-Agent}i"'
SHAPES = sorted(fx.SHAPES.items())


def paths(fmt):
    return lpa.get_possible_paths(fmt)


@pytest.fixture(scope="module")
def plans():
    return {name: fx.Fixed(name, paths(name)) for name, _ in SHAPES}


def to_common(line):
    """the common-format part of a combined line"""
    return line.rsplit(b' "', 2)[0]


@pytest.fixture(scope="module")
def synth_lines():
    """the first 200 K lines of synthetic workload 2"""
    return lpa.synth(lpa.SYNTH_COMBINED, 20261015, 0, 200_000).split(b"\n")[:-1]


def lines_of(name, lines):
    return lines if name == "combined" else [to_common(l) for l in lines]


# ------------------------------------------------------------- table drift
@pytest.mark.parametrize("name,shape", SHAPES)
def test_table_equals_compiled_program(plans, name, shape):
    n, what = plans[name].table_diff(shape)
    assert n == 0, what
    assert plans[name].shape() == shape


def test_written_out_format_is_the_shape():
    """the predicate looks at the Program, not at the format's name"""
    assert fx.Fixed(COMBINED, paths(COMBINED)).shape() == fx.SHAPES["combined"]


@pytest.mark.parametrize("fmt", [
    COMBINED.replace('"%{User-Agent}i"', "'%{User-Agent}i'"),   # one literal changed
    COMBINED.replace("%>s %b", "%>s  %b"),                      # ... by one byte
    COMBINED + " %D",                                           # one field added
    "combinedio",
    "combined\ncommon",                                         # a two-format handle
], ids=["literal", "literal-byte", "field-added", "combinedio", "two-formats"])
def test_near_miss_is_refused(fmt):
    f = fx.Fixed(fmt, paths(fmt))
    assert f.shape() == 0
    for _, shape in SHAPES:
        assert f.table_diff(shape)[0] > 0


@pytest.mark.parametrize("name,shape", SHAPES)
def test_field_subset_is_refused(name, shape):
    """fewer requested paths change the capture slots and the stage lists,
    which the instance holds as constants: the generic instances take them"""
    for fields in (["IP:connection.client.host"], ["TIME.EPOCH:request.receive.time.epoch"],
                   ["HTTP.METHOD:request.firstline.method", "STRING:request.status.last"]):
        assert fx.Fixed(name, fields).shape() == 0, fields


# ------------------------------------------------------------ differential
def check(plan, shape, lines, off=-1, want=("ok",)):
    data = b"\n".join(lines) + b"\n"
    n, stats, first = plan.diff(shape, data, off)
    assert n == 0, (first, stats)
    assert stats["lines"] == len(lines)
    for k in want:
        assert stats[k] > 0, stats
    return stats


@pytest.mark.parametrize("name,shape", SHAPES)
def test_differential_synth(plans, synth_lines, name, shape):
    stats = check(plans[name], shape, lines_of(name, synth_lines))
    assert stats["ok"] == len(synth_lines), stats


@pytest.mark.parametrize("name,shape", SHAPES)
def test_differential_corpora(plans, synth_lines, demolog_lines, name, shape):
    base = synth_lines[:3000]
    check(plans[name], shape, lines_of(name, corpora.utf8_ua_lines(base, 1)))
    # (the hard UTF-8 sits mostly in the referer and user agent, which a common line does not have)
    check(plans[name], shape, lines_of(name, corpora.utf8_hard_lines(base, 2)),
          want=("ok", "fallback") if name == "combined" else ("ok",))
    check(plans[name], shape, lines_of(name, demolog_lines))
    # the other shape's lines, and lines with their terminator's '\r' left on
    other = "common" if name == "combined" else "combined"
    check(plans[name], shape, lines_of(other, base), want=("lines",))
    check(plans[name], shape, [l + b"\r" for l in lines_of(name, base[:500])], want=("lines",))


@pytest.mark.parametrize("name,shape", SHAPES)
def test_differential_adversarial_every_window_offset(plans, name, shape):
    """each adversarial line at every offset of its 64-byte window, so quotes
    and spaces fall on bits 63 and 0 of a mask word; a line whose first leaf
    fails fails in both (REDO / BAD unchanged)"""
    adv = fx.adversarial(shape)
    assert len(adv) > 300 and any(len(l) == 8192 for l in adv) and b"" in adv
    for off in range(64):
        check(plans[name], shape, adv, off, want=("ok", "bad", "redo", "fallback"))


def test_sanitized_standalone_program():
    """the adversarial set through the host build of both matchers under
    ASan + UBSan: a program with its own main, run directly"""
    r = subprocess.run([fx.build_sanitized_main()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "combined:" in r.stdout and "common:" in r.stdout and " 0 differ" in r.stdout, r.stdout
