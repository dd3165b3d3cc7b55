"""Timestamp fill of the fused scan (k_rle_ts_tiles: work split by tiles of
output rows, timestamps from the span table of k_spans_rle), through
Engine.scan and scan_fields_async.

Expected timestamps are numpy slices of the generating arange, compared as
exact int64; values are checked bit-exact against the oracle's decode of
the same pages.  Output buffers are longer than the result and pre-filled
with a sentinel that must survive everywhere outside the result.

Shapes: pages of 2, 3, every candidate tile (4096, 8192, 16384) -1/+0/+1
and 40000 rows, the list rotated per series, so groups start and end on,
one before and one after tile edges, thousands of rows apart and two rows
apart; deltas of 1 s, 10 s (power-of-ten scaler), 7 ns and 0 (constant
pages) in one set.  One-row time pages are not RLE and stay out, as in
test_gpu_gor_loop.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ts_sets as S  # noqa: E402
from ts_sets import NS, T0, PAGE_FIRST  # noqa: E402

pytestmark = pytest.mark.gpu


def _rows(a, b):
    """Closed time range that selects rows a..b of series 0 (1 s apart),
    starting and ending between two rows."""
    return T0 + a * NS - NS // 2, T0 + b * NS + NS // 3


# name -> closed time range
RANGES = {
    "everything": (T0 - NS, T0 + 2_000_000 * NS),
    "before the set": (T0 - 500 * NS, T0 - 100 * NS),
    "after the set": (T0 + 3_000_000 * NS, T0 + 4_000_000 * NS),
    # 7001 s is no multiple of 10 s and lies before the 7 ns series
    "a single row": (T0 + 7001 * NS, T0 + 7001 * NS),
    # series 0 contributes N_ALL-5 and N_ALL-6 rows, an even and an odd
    # count: every group behind it moves by one output row between the two,
    # so each meets the 16-B store peel once with and once without a head
    "start row 5": _rows(5, 2_000_000),
    "start row 6": _rows(6, 2_000_000),
    "end on a page's first row": (T0 - NS, T0 + int(PAGE_FIRST[5]) * NS),
    "end on a page's last row": (T0 - NS, T0 + int(PAGE_FIRST[5] - 1) * NS),
    # cuts the 7 ns series at rows 1000 and 99999
    "inside the 7 ns series": (T0 + 60_000 * NS + 7 * 1000,
                               T0 + 60_000 * NS + 7 * 99_999 + 3),
    "mid pages": _rows(4100, 100_000),
}


@pytest.fixture(scope="module")
def engine():
    import cnosdb_amd as gs
    e = gs.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tile_set(engine):
    groups, truth = S.groups_of(S.tile_series(), 1, seed=11)
    assert len(truth) == 4, "the encoder no longer makes constant pages RLE"
    sc = S.Scanner(engine, groups, 1)
    yield sc, truth
    sc.free()


@pytest.mark.parametrize("name", list(RANGES))
def test_ranges(tile_set, name):
    sc, truth = tile_set
    lo, hi = RANGES[name]
    exp = S.expect(truth, 1, lo, hi)
    if name in ("before the set", "after the set"):
        assert exp["ts"].size == 0
    if name == "a single row":
        assert exp["ts"].size == 1
    sc.launch(lo, hi)
    S.check(sc.wait(), exp, f"{name} async")
    S.check(sc.scan_sync(lo, hi), exp, f"{name} sync")


@pytest.mark.parametrize("name", ["everything", "start row 5", "start row 6",
                                  "a single row", "before the set"])
def test_unaligned_destination(tile_set, name):
    """d_out_ts[1:] is 8-B-aligned but not 16-B-aligned; element 0 and
    everything past the result keep the sentinel."""
    sc, truth = tile_set
    assert sc.d_ots.data_ptr() % 16 == 0
    lo, hi = RANGES[name]
    exp = S.expect(truth, 1, lo, hi)
    sc.launch(lo, hi, offset=1)
    got = sc.wait(offset=1)
    assert got["ts_before"].size == 1
    S.check(got, exp, f"{name} async, offset 1")
    S.check(sc.scan_sync(lo, hi, offset=1), exp, f"{name} sync, offset 1")


def test_no_stale_rows(tile_set):
    """Two ranges in a row into the same buffers, without clearing them:
    the second result holds the second range only."""
    sc, truth = tile_set
    a, b = RANGES["everything"], RANGES["mid pages"]
    sc.launch(*a)
    S.check(sc.wait(), S.expect(truth, 1, *a), "first range")
    sc.launch(*b, refill=False)
    S.check(sc.wait(), S.expect(truth, 1, *b), "second range",
            sentinels=False)
    c = RANGES["inside the 7 ns series"]
    sc.launch(*c, refill=False)
    S.check(sc.wait(), S.expect(truth, 1, *c), "third range",
            sentinels=False)


def test_runs_of_empty_groups_inside_a_tile(engine):
    """400 groups of 100 rows; the groups with g % 4 == 0 lie in the
    selected hour, the others a year later: a tile of the output holds
    dozens of groups with runs of three empty ones between them.  Then the
    complement, which starts and ends with selected groups after one empty
    one."""
    late = 365 * 86400 * NS
    series = []
    for g in range(400):
        start = (g * 7) * NS + (0 if g % 4 == 0 else late)
        series.append((g, [T0 + start
                           + np.arange(100, dtype=np.int64) * NS]))
    groups, truth = S.groups_of(series, 1, seed=5)
    sc = S.Scanner(engine, groups, 1)
    try:
        for lo, hi in ((T0 - NS, T0 + 3600 * NS),
                       (T0 + late - NS, T0 + late + 3600 * NS)):
            exp = S.expect(truth, 1, lo, hi)
            assert exp["ts"].size in (100 * 100, 300 * 100)
            sc.launch(lo, hi)
            S.check(sc.wait(), exp, "alternate groups")
    finally:
        sc.free()


def test_two_row_pages(engine):
    """4500 pages of 2 rows and one of 3: thousands of groups inside one
    tile, cut by a range in the middle of a page."""
    rows = [2] * 4500 + [3]
    ts = T0 + np.arange(sum(rows), dtype=np.int64) * NS
    groups, truth = S.groups_of([(0, S.split(ts, rows))], 1, seed=6)
    sc = S.Scanner(engine, groups, 1)
    try:
        for lo, hi in ((T0 - NS, T0 + 10**6 * NS), _rows(1, 8999),
                       _rows(4001, 4001)):
            sc.launch(lo, hi)
            S.check(sc.wait(), S.expect(truth, 1, lo, hi), "2-row pages")
    finally:
        sc.free()


def test_aliasing_shape_in_small(engine):
    """512 series x 8 pages x 64 rows, pages 2..5 of every series
    selected: the shape at which one block per page left half the grid
    without work.  Correctness only."""
    series = []
    for s in range(512):
        ts = T0 + np.arange(8 * 64, dtype=np.int64) * NS
        series.append((s, S.split(ts, [64] * 8)))
    groups, truth = S.groups_of(series, 1, seed=7)
    sc = S.Scanner(engine, groups, 1)
    try:
        lo, hi = _rows(2 * 64, 6 * 64 - 1)
        exp = S.expect(truth, 1, lo, hi)
        assert exp["ts"].size == 512 * 4 * 64
        sc.launch(lo, hi)
        S.check(sc.wait(), exp, "aliasing shape")
    finally:
        sc.free()
