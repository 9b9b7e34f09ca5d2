"""The owner lookup of the URI kernels' cooperative passes (lp_owner.h) on the
CPU: for vectors of per-lane item counts, the helper's owner of every item
against the definition, the last lane whose first item is <= the item
(tests/emu/owner_emu.cpp)."""
import functools
import subprocess

import pytest

import owner_emu_lib as ow

# vectors per group: 3 lanes x 6 counts; 3 lane pairs x 5 x 5; 2 x 3 x 2 x 3; 8 totals x 4 layouts
VECTORS = {"all-ones": 1, "single-lane": 18, "lane-pairs": 75, "empty-runs": 36, "totals": 32, "random": 20000}


@functools.lru_cache(None)
def _run(name):
    return ow.run_group(name)


def test_groups_are_the_listed_ones():
    assert ow.groups() == list(VECTORS)


@pytest.mark.parametrize("name", list(VECTORS))
def test_owner_equals_definition(name):
    n, stats, first = _run(name)
    assert n == 0, first
    assert stats["vectors"] == VECTORS[name], stats
    assert stats["items"] > 0 and stats["rounds"] > 0, stats


def test_groups_reach_their_boundaries():
    """rounds without any head (a lane with more than 64 items) occur in the
    groups meant to have them, and the random group has many"""
    for name in ("single-lane", "lane-pairs", "empty-runs", "random"):
        assert _run(name)[1]["empty_rounds"] > 0, name
    assert _run("all-ones")[1] == {"vectors": 1, "items": 64, "rounds": 1, "empty_rounds": 0}
    assert _run("random")[1]["items"] > 20000 * 64 * 10


def test_vectors_given_from_python():
    """a few vectors spelled out here: the count of items checked is the vector's sum"""
    for counts in ([1] * 64, [0] * 63 + [600], [64] + [0] * 40 + [1] + [0] * 22, [0] * 64,
                   [130, 0, 0, 62, 0, 1] + [0] * 57 + [5]):
        n, items, first = ow.check(counts)
        assert n == 0, first
        assert items == sum(counts)


def test_sanitized_standalone_program():
    """every group through a host build under ASan + UBSan: a program with its own main, run directly"""
    r = subprocess.run([ow.build_sanitized_main()], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in VECTORS:
        assert name + ":" in r.stdout, r.stdout
    assert r.stdout.count(" 0 differ") == len(VECTORS), r.stdout
