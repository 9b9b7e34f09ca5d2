"""Sticky multi-format routing on overlapping formats, GPU part: the routing
scan (k_fmt_reduce / k_fmt_chunks / k_fmt_apply), the lines the chunk kernel
queues for it (k_route_ovf, k_parse_ovf_lines), the handle's state from batch
to batch and through the capacity and arena re-runs, and what reads the routed
format afterwards (the typed table's per-format sources, the histograms).

The corpus (sticky_corpus.py) is four Apache formats whose match sets overlap,
so the routed format depends on the routing state and shows in the record; the
sequences put state changes, overlapping runs, failing and undecided lines at
the scan's edges (64 lines per lane, 4096 per chunk) and at batch ends.  The
expectation of every line is sticky_corpus.fold(), a left fold written from
the Java rule, with records from four single-format oracles; per line the
status class, the record, the routed format (fmt_id) and the counters are
compared.  Lines the fold leaves undecided are at most 10 % of a sequence
(asserted from the fold alone), so a scan that lost its state cannot hide in
skipped lines.  The CPU part (the fold against the stateful oracle, the
emulation, the scan's algebra) is test_sticky_routing.py."""
import numpy as np
import pytest

import logparser_amd as lpa
import sticky_corpus as sc

pytestmark = pytest.mark.gpu

SEQUENCES = sc.sequences()
STATUS_OF = {sc.OK: (lpa.LINE_OK,), sc.BAD: (lpa.LINE_BAD,), sc.FALLBACK: (lpa.LINE_FALLBACK,),
             sc.BAD_OR_FALLBACK: (lpa.LINE_BAD, lpa.LINE_FALLBACK)}
STATUS, BYTES, MICROS = ("STRING:request.status.last", "BYTES:response.body.bytes",
                         "MICROSECONDS:response.server.processing.time")


@pytest.fixture(scope="module")
def records(oracle):
    return sc.Records(oracle)


@pytest.fixture(scope="module")
def fields(oracle):
    return oracle.possible_paths(sc.LOGFORMAT)


@pytest.fixture(scope="module")
def handle(fields):
    """one handle for the module; reset() brings its routing state to 0 whatever ran before"""
    return lpa.HttpdLoglineParser(sc.LOGFORMAT, fields)


def reset(p):
    r = p.parse_batch(sc.make_line("X0", 0) + b"\n")
    assert r.n_lines == 1 and r.status[0] == lpa.LINE_OK
    return p


def join(lines, last_newline=True):
    data = b"".join(l + b"\n" for l in lines)
    return data if last_newline or not data else data[:-1]


def check_batch(r, lines, rows, records):
    """one batch's results against the fold's rows of its lines"""
    n = len(lines)
    assert r.n_lines == n
    status = r.status
    for i, (line, row) in enumerate(zip(lines, rows)):
        assert int(status[i]) in STATUS_OF[row.cls], (i, line, row, int(status[i]))
        if row.cls == sc.OK:
            assert sc.same_record(r.record_json(i), records.record_json(row.fmt, line)), (i, line, row)
    if n:
        _, res = r.copy_to_host(with_input=False)
        fmt_id = r.columns(res)[("fmt_id", 0)][:n]
        want = np.array(sc.fmt_ids(rows), dtype=np.uint8)
        bad = np.flatnonzero(fmt_id != want)
        assert bad.size == 0, [(int(i), int(fmt_id[i]), int(want[i])) for i in bad[:10]]
    c = r.counters
    assert c["lines"] == n
    assert (c["ok"], c["bad"], c["fallback"]) == tuple(int((status == s).sum()) for s in (0, 1, 2)), c


def run_sequence(p, batches, records, last_newline=True, **line_kw):
    """the batches through the handle in order, against one fold over their concatenation from
    state 0"""
    kinds = [k for b in batches for k in b]
    rows = sc.fold(kinds)
    assert sc.undecided_share(rows) <= 0.10
    first = 0
    for b in batches:
        lines = sc.make_lines(b, first, **line_kw)
        r = p.parse_batch(join(lines, last_newline))
        check_batch(r, lines, rows[first:first + len(b)], records)
        first += len(b)


ONE_BATCH = sorted(n for n, b in SEQUENCES.items() if len(b) == 1)
BATCHES = sorted(n for n, b in SEQUENCES.items() if len(b) > 1 and not n.startswith("count-"))


@pytest.mark.parametrize("name", ONE_BATCH)
def test_one_batch(handle, records, name):
    """state changes, failing and undecided lines at the lane and chunk edges, lanes and chunks
    that only compose, every transition, all lines queued / none, random kinds"""
    run_sequence(reset(handle), SEQUENCES[name], records)


@pytest.mark.parametrize("newline", [True, False])
@pytest.mark.parametrize("n", sc.COUNTS)
def test_line_counts(handle, records, n, newline):
    """n lines (X3 ... A) after a batch that left state 1, with and without the last newline"""
    run_sequence(reset(handle), SEQUENCES["count-%d" % n], records, last_newline=newline)


@pytest.mark.parametrize("name", BATCHES)
def test_batches(handle, records, name):
    """the state from batch to batch: splits at the lane and chunk sizes, batches that end on an
    overlapping, a failing, an undecided and an exclusive line, an empty batch in between"""
    run_sequence(reset(handle), SEQUENCES[name], records)


def test_fresh_handle_starts_at_format_0(fields, records):
    p = lpa.HttpdLoglineParser(sc.LOGFORMAT, fields)
    run_sequence(p, [["A"] * 70 + ["X3"] + ["B"] * 70], records)


def test_capacity_rerun(fields, records):
    """a batch of long lines, then many short ones: the second outgrows the columns sized from the
    first and is re-run inside lp_sync; the re-run starts from the state the first batch left (3),
    the third batch from the state the second left (1)"""
    p = lpa.HttpdLoglineParser(sc.LOGFORMAT, fields)
    long_kinds = sc.keeping(300, {0: "X1", 299: "X3"})
    short_kinds = sc.keeping(8000, {5000: "X2", 7999: "X1"}, state=3)
    after = sc.keeping(200, {}, state=1)
    rows = sc.fold(long_kinds + short_kinds + after)
    assert rows[300].state == 3 and rows[8299].state == 1 and rows[8300].fmt == 1 and sc.undecided_share(rows) == 0
    first = 0
    for kinds, pad in ((long_kinds, 900), (short_kinds, 0), (after, 0)):
        lines = sc.make_lines(kinds, first, pad=pad)
        r = p.parse_batch(join(lines))
        assert (r.diag["retries"] > 0) == (kinds is short_kinds), r.diag
        check_batch(r, lines, rows[first:first + len(kinds)], records)
        first += len(kinds)


def test_arena_rerun(fields, records):
    """a far too small arena (LP_OPT_ARENA_BYTES) and query strings on every request: the second
    batch is re-run inside lp_sync with the exact arena; the re-run starts from the state before
    the batch (3, left by the first batch's last line), the third batch from the state after it"""
    p = lpa.HttpdLoglineParser(sc.LOGFORMAT, fields, reserve_arena=4096, options={lpa.OPT_ARENA_BYTES: 64 * 1024})
    b0 = sc.keeping(100, {0: "X1", 99: "X3"})
    b1 = sc.keeping(6000, {3000: "N", 4500: "X0", 5999: "X1"}, state=3)
    b2 = sc.keeping(200, {100: "X2"}, state=1)
    rows = sc.fold(b0 + b1 + b2)
    assert rows[100].fmt == 3 and rows[6100].fmt == 1 and sc.undecided_share(rows) == 0
    first = 0
    for kinds in (b0, b1, b2):
        lines = sc.make_lines(kinds, first, query=kinds is b1)
        r = p.parse_batch(join(lines))
        if kinds is b1:
            assert r.diag["retries"] > 0 and r.diag["arena_ovf"] == 0, r.diag
        check_batch(r, lines, rows[first:first + len(kinds)], records)
        first += len(kinds)


# ---------------------------------------------------------------- the other outputs
@pytest.fixture(scope="module")
def random_batch(fields, records):
    """the random sequence parsed once by a handle of its own (its readers below need the batch to
    stay the handle's last), with the fold's rows and the expected records of its OK lines"""
    kinds = SEQUENCES["random"][0]
    rows = sc.fold(kinds)
    lines = sc.make_lines(kinds)
    p = lpa.HttpdLoglineParser(sc.LOGFORMAT, fields)
    r = p.parse_batch(join(lines))
    recs = [records.record(row.fmt, line) if row.cls == sc.OK else None for line, row in zip(lines, rows)]
    return p, r, rows, recs


def _last(rec, path):
    v = rec.get(path, [None])[-1] if rec else None
    return v["l"] if isinstance(v, dict) else v


def _expected_columns(recs):
    """(values, valid) per path of the three table columns from the fold's records: the status as
    text, the bytes and the %D microseconds as longs (no value: not an OK line, or F0 / F1's %D)"""
    out = {}
    for path, typ in ((STATUS, str), (BYTES, int), (MICROS, int)):
        vals = [_last(rec, path) for rec in recs]
        out[path] = ([v if v is None or typ is str else int(v) for v in vals], [v is not None for v in vals])
    return out


def _check_table(t, want, rows_idx, device):
    for path, (vals, valid) in want.items():
        got, ok = t[path]
        if device:
            ok = ok.cpu().numpy().astype(bool)
            if path == STATUS:
                off, chars = (x.cpu().numpy() for x in got)
                chars = chars.tobytes()
                got = [chars[off[j]:off[j + 1]].decode() for j in range(len(rows_idx))]
            else:
                got = got.cpu().numpy()
        assert list(ok[:len(rows_idx)]) == [valid[i] for i in rows_idx], path
        for j, i in enumerate(rows_idx):
            if valid[i]:
                assert got[j] == vals[i], (path, j, i, got[j], vals[i])


def test_typed_table(random_batch):
    """lp_result_table on a status, a bytes and a %D column (the per-format sources the routed
    format selects; %D null for F0 / F1) against the fold's records: a window from the host copy
    and on the device, and the OK lines through lp_result_select + lp_result_table_rows"""
    p, r, rows, recs = random_batch
    cols = [(STATUS, str), (BYTES, int), (MICROS, int)]
    want = _expected_columns(recs)
    ok_lines = [i for i, row in enumerate(rows) if row.cls == sc.OK]
    assert {rows[i].fmt for i in ok_lines} == {0, 1, 2, 3}
    assert 0 < sum(want[MICROS][1]) < len(ok_lines)
    _, res = r.copy_to_host()
    window = list(range(100, 5900))
    _check_table(r.table_from(res, cols, first=100, count=5800), want, window, False)
    _check_table(r.table_device(cols, first=100, count=5800), want, window, True)
    sel = r.select_from(res, lpa.SEL_OK)
    assert sel.tolist() == ok_lines
    _check_table(r.table_from(res, cols, rows=sel), want, ok_lines, False)
    dsel = r.select_device(lpa.SEL_OK)
    assert dsel.cpu().numpy().tolist() == ok_lines
    _check_table(r.table_device(cols, rows=dsel), want, ok_lines, True)


def test_histograms(random_batch):
    """lp_histograms of a multi-format batch: the line counts (words 0-3), the status codes (the
    routed format's %>s token: on an A line 200 under F0, n under F1) and the methods, against
    counts from the fold's records.  The per-token null / present words (16-47) are left out:
    their layout for several formats is not restated here."""
    p, r, rows, recs = random_batch
    want = np.zeros(lpa.HIST_WORDS, dtype=np.int64)
    want[0] = len(rows)
    for i, (row, rec) in enumerate(zip(rows, recs)):
        st = int(r.status[i])
        assert st in STATUS_OF[row.cls], (i, row, st)  # (a failing line of an unknown state: either)
        want[1 + st] += 1
        if rec is None:
            continue
        s = _last(rec, STATUS)
        if s is not None and len(s) == 3 and s.isdigit() and 100 <= int(s) <= 599:
            want[100 + int(s)] += 1
        else:
            want[48] += 1
        m = _last(rec, "HTTP.METHOD:request.firstline.method")
        if not m:
            want[64 + 16] += 1
        else:
            want[64 + (lpa.HIST_METHODS.index(m) if m in lpa.HIST_METHODS[:15] else 15)] += 1
    got = np.array(p.histograms(), dtype=np.int64)
    got[16:48] = 0
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(w), int(got[w]), int(want[w])) for w in bad[:20]]
    d = lpa.decode_histograms(got)
    assert len(d["methods"]) >= 5 and len(d["status"]) > 50 and d["status_other"] > 500, d
