"""Corpora of the URI kernels' dense decode pass (decode_wave_corpus), GPU
part: the piece pass of uri_wave (uri.hip) hands every query value that holds
a '%' / '+' to a lane of its own through a descriptor buffer of CAPD entries.
Every line against the oracle, bit-exact, none FALLBACK, on the compact path
and on the direct one; the CPU part (the corpora's self-checks, the serial
code on the same lines) is test_decode_wave.py."""
import functools

import pytest

import decode_wave_corpus as dwc
import logparser_amd as lpa
from test_gpu_parity import _device_vs_host_table
from test_uri_wave_gpu import _parser, decided, decided_with

pytestmark = pytest.mark.gpu


@functools.lru_cache(None)
def _cases():
    return {c.name: c for c in dwc.all_cases()}


NAMES = ["N-counts", "P-placement", "V-values", "V-long2000", "V-long6000", "M-names"]


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_dense_decode_gpu(oracle, name, direct):
    """N: 0..256 values to decode in one 256-piece round, around the buffer's
    capacity, and a full block arriving when one value waits; P: their
    placement in the round, the line and the two URI stages, and across a
    round boundary; V: what is decoded, every padding of the last word, a
    2,000-byte value among 1-byte ones (no wave leaves the compact path) and a
    6,000-byte one (k_uri_overflow's buffer); M: rewritten names before
    decoded values."""
    c = _cases()[name]
    p = _parser(oracle, c, options={lpa.OPT_FORCE_DIRECT: direct})
    r = decided_with(oracle, c, p)
    assert r.counters["ok"] == len(c.lines)
    print("%s direct=%d: pv per block %s, uri_overflow_waves %d" % (name, direct, c.info["pv"], r.diag["uri_overflow_waves"]))
    if not direct and name != "V-long6000":
        assert r.diag["uri_overflow_waves"] == 0, r.diag
    if not direct and name == "V-long6000":
        assert r.diag["uri_overflow_waves"] == 1, r.diag


@pytest.mark.parametrize("direct", [0, 1])
def test_unwanted_values_gpu(oracle, direct):
    """one named parameter: the other pieces' slots are skips, their values
    are not decoded"""
    for name in ("N-counts", "M-names"):
        c = _cases()[name]
        p = _parser(oracle, c, fields=dwc.NAMED_FIELDS, options={lpa.OPT_FORCE_DIRECT: direct})
        decided_with(oracle, c, p)


def test_several_formats_gpu(oracle):
    """lanes of three LogFormats share the piece blocks and the decode pass
    (the SLOT instance)"""
    from test_emu_parity import mixed_lines
    c = dwc.mixed_decode_case(mixed_lines(512, 62))
    r = decided(oracle, c, options={lpa.OPT_ONE_PASS: 1})
    assert r.counters["ok"] > 450


def test_reused_handle_gpu(oracle):
    """one handle over three different cases, and the first again: no
    descriptor, slot or spill of an earlier batch is read"""
    a, b, c = (_cases()[n] for n in ("N-counts", "V-values", "M-names"))
    p = _parser(oracle, a)
    for x in (a, b, c, a):
        decided_with(oracle, x, p)


def test_value_columns_device_table_gpu(oracle):
    """table.hip reads the slots and the decoded bytes the pass wrote: the
    device table equals the host table on the value family's query-parameter
    and query-string columns"""
    c = _cases()["V-values"]
    p = lpa.HttpdLoglineParser("combined", lpa.get_possible_paths("combined"))
    r = p.parse_batch(c.data)
    assert r.counters["ok"] == len(c.lines) and r.diag["arena_ovf"] == 0, (r.counters, r.diag)
    _, res = r.copy_to_host()
    cols = [(f, str) for f in ("STRING:request.firstline.uri.query.k7", "STRING:request.firstline.uri.query.x",
                               "STRING:request.referer.query.q", "HTTP.QUERYSTRING:request.firstline.uri.query",
                               "HTTP.QUERYSTRING:request.referer.query")]
    assert _device_vs_host_table(r, res, cols) == []
