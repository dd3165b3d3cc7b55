"""What gs_agg_group must compute, restated from the contract in
include/cnosdb_gs.h on top of filter_ref's keep mask and effective validity,
and the designed cases of its tests.

The restatement knows rows only: no segments, no runs, no partials.  A cell
is reduced by one sequential loop over its rows in row order: integers are
Python ints reduced modulo 2**64 at the end, min / max are strict compares
(so a NaN never enters a bound and the first of +0.0 / -0.0 stays), first /
last follow the timestamps with the row order breaking ties, and the f64 sum
is math.fsum, the correctly rounded sum, against which any summation order
is held to the standard bound n * 2^-53 * sum|x|.

HAND is hand-written: every expected cell in it was worked out by a person
from the contract, not produced by any code.  tests/test_agg_ref_cpu.py holds
`agg_ref` to it; the host check (tests/cpu/agg_check.cpp) and the device
then have to agree with both.

Built from numpy alone.  Not a test module and not a conftest."""
import math
import os
import struct
import subprocess
from collections import namedtuple

import numpy as np

import filter_ref as fr
from filter_ref import (CT_BOOL, CT_F64, CT_I64, CT_U64, I64_MAX, I64_MIN,
                        INF, NAN)
from str_corpus import SANITIZE, host_compiler

NAMES = ("count", "sum", "min", "max", "first", "last", "first_ts", "last_ts")
M64 = 2**64 - 1
NEG0 = 0x8000000000000000          # bits of -0.0
NAN_BITS = fr.bits(CT_F64, NAN)

# a filter case plus the aggregate's own arguments.  aggs = [(col, names)],
# col an index into case.cols; series = rows per series (None: case.sizes,
# the raw set of the case)
AggCase = namedtuple("AggCase", "case aggs t0 bucket_ns n_buckets per_series "
                                "series", defaults=(None,))

# ---------------------------------------------------------------- the rules


def bucket_of(ts, t0, bucket_ns, n_buckets):
    """The bucket of a timestamp, None for a row in no bucket.  Python ints:
    nothing can overflow."""
    ts, t0 = int(ts), int(t0)
    if bucket_ns == 0:
        return 0
    if ts < t0:
        return None
    b = (ts - t0) // int(bucket_ns)
    return b if b < n_buckets else None


def value_of(ctype, bits):
    """Raw bits as the value the compares see."""
    if ctype == CT_F64:
        return struct.unpack("<d", struct.pack("<Q", bits))[0]
    if ctype == CT_I64:
        return bits - 2**64 if bits >= 2**63 else bits
    return bits


def empty_cell(ctype):
    mn, mx = {CT_F64: (fr.bits(CT_F64, INF), fr.bits(CT_F64, -INF)),
              CT_I64: (I64_MAX, I64_MIN & M64),
              CT_BOOL: (1, 0),
              CT_U64: (M64, 0)}[ctype]
    return {"count": 0, "sum": 0, "min": mn, "max": mx, "first": 0,
            "last": 0, "first_ts": I64_MAX, "last_ts": I64_MIN,
            "sum_abs": 0.0}


def reduce_rows(ctype, rows):
    """One cell: rows = [(ts, bits)] of its kept, effectively valid cells in
    row order.  Values come back as raw 64-bit patterns (count and the two
    timestamps as ints); for f64, sum is the bits of math.fsum and sum_abs
    the exact sum of |x| for the tolerance."""
    c = empty_cell(ctype)
    mn = value_of(ctype, c["min"])
    mx = value_of(ctype, c["max"])
    isum, fvals = 0, []
    for ts, bits in rows:
        x = value_of(ctype, bits)
        c["count"] += 1
        if ctype == CT_F64:
            fvals.append(x)
        else:
            isum += x
        if x < mn:                      # strict: NaN and equal values fail
            mn, c["min"] = x, bits
        if x > mx:
            mx, c["max"] = x, bits
        if ts < c["first_ts"] or c["count"] == 1:
            c["first"], c["first_ts"] = bits, ts
        if ts >= c["last_ts"]:
            c["last"], c["last_ts"] = bits, ts
    if ctype == CT_F64:
        if any(math.isnan(v) for v in fvals) or (
                INF in fvals and -INF in fvals):
            total = NAN
        else:
            total = math.fsum(fvals)
        c["sum"] = fr.bits(CT_F64, total)
        c["sum_abs"] = math.fsum(abs(v) for v in fvals)
    else:
        c["sum"] = isum % 2**64
    return c


def series_of_rows(sizes):
    return np.repeat(np.arange(len(sizes)), np.asarray(sizes, dtype=np.int64))


def cell_rows(ac):
    """(cells, rows of every cell in set order): the kept rows that lie in a
    bucket.  With per_series the cell is series * n_buckets + bucket, else
    the bucket."""
    case = ac.case
    sizes = list(ac.series if ac.series is not None else case.sizes)
    keep = fr.filter_ref(case).keep
    ser = series_of_rows(sizes)
    ncell = (len(sizes) if ac.per_series else 1) * ac.n_buckets
    out = [[] for _ in range(ncell)]
    for r in np.flatnonzero(keep):
        b = bucket_of(case.ts[r], ac.t0, ac.bucket_ns, ac.n_buckets)
        if b is None:
            continue
        out[(int(ser[r]) * ac.n_buckets if ac.per_series else 0) + b].append(
            int(r))
    return ncell, out


def agg_ref(ac):
    """{"rows": [kept rows per cell], "cols": [per aggregated column a dict
    name -> list over the cells]} with every aggregate of every column,
    wanted or not."""
    case = ac.case
    ts = np.asarray(case.ts, dtype=np.int64)
    ncell, rows = cell_rows(ac)
    out = {"rows": [len(r) for r in rows], "cols": []}
    for col, _ in ac.aggs:
        c = case.cols[col]
        ev = fr.effective(c, ts)
        res = {n: [] for n in NAMES + ("sum_abs",)}
        for cell in rows:
            red = reduce_rows(c.ctype, [(int(ts[r]), fr.bits(c.ctype, c.val[r]))
                                        for r in cell if ev[r]])
            for n in res:
                res[n].append(red[n])
        out["cols"].append(res)
    return out


def sum_within(ctype, got_bits, ref_bits, count, sum_abs):
    """The f64 sum rule: |got - fsum| <= n * 2^-53 * sum|x| (any summation
    order of n values); a NaN or infinite reference must be matched in kind.
    Integer sums are exact."""
    if ctype != CT_F64:
        return got_bits == ref_bits
    got, ref = value_of(CT_F64, got_bits), value_of(CT_F64, ref_bits)
    if math.isnan(ref) or math.isnan(got):
        return math.isnan(ref) and math.isnan(got)
    if math.isinf(ref) or math.isinf(got):
        return got == ref
    return abs(got - ref) <= count * 2.0**-53 * sum_abs


# ------------------------------------------------------- the hand-written table
# One aggregated column (column 0) per case.  `want` lists every aggregate of
# every cell as a person reads it off the rows: f64 values as floats (NaN by
# name), integers as ints, bits(-0.0) spelled NEG0.

Hand = namedtuple("Hand", "name ac want")
_E_I64 = dict(count=0, sum=0, min=I64_MAX, max=I64_MIN, first=0, last=0,
              first_ts=I64_MAX, last_ts=I64_MIN)
_E_F64 = dict(count=0, sum=0.0, min=INF, max=-INF, first=0, last=0,
              first_ts=I64_MAX, last_ts=I64_MIN)
_E_U64 = dict(count=0, sum=0, min=2**64 - 1, max=0, first=0, last=0,
              first_ts=I64_MAX, last_ts=I64_MIN)
_E_BOOL = dict(count=0, sum=0, min=1, max=0, first=0, last=0,
               first_ts=I64_MAX, last_ts=I64_MIN)


def _cell(count, total, mn, mx, first, last, first_ts, last_ts):
    return dict(count=count, sum=total, min=mn, max=mx, first=first,
                last=last, first_ts=first_ts, last_ts=last_ts)


def _hand(name, sizes, ts, cols, want_rows, cells, preds=(), time_range=None,
          row_tombs=(), t0=100, bucket_ns=10, n_buckets=2, per_series=True):
    case = fr.Case(name, sizes, np.array(ts, np.int64), cols, [], list(preds),
                   time_range, list(row_tombs))
    ac = AggCase(case, [(0, NAMES)], t0, bucket_ns, n_buckets, per_series)
    return Hand(name, ac, {"rows": want_rows, "cells": cells})


def _f(v, valid=None, tombs=()):
    return fr.Col(CT_F64, np.array(v, np.float64),
                  None if valid is None else np.array(valid, bool), tombs)


def _i(v, valid=None, tombs=()):
    return fr.Col(CT_I64, np.array(v, np.int64),
                  None if valid is None else np.array(valid, bool), tombs)


HAND = [
    # buckets [100,110) and [110,120).  The range drops ts 100 although it
    # lies in bucket 0 (a range edge inside a bucket) and ts 95 / 120; the
    # row tombstone removes ts 110; ts 103 is a null cell and ts 114 lies in
    # the column's deleted range: both rows are kept and counted in `rows`,
    # neither in `count`.
    _hand("null_tombstones_range", [8],
          [95, 100, 103, 109, 110, 114, 119, 120],
          [_f([1, 2, 4, 8, 16, 32, 64, 128], [1, 1, 0, 1, 1, 1, 1, 1],
              [(114, 114)])],
          [2, 2],
          [_cell(1, 8.0, 8.0, 8.0, 8.0, 8.0, 109, 109),
           _cell(1, 64.0, 64.0, 64.0, 64.0, 64.0, 119, 119)],
          time_range=(101, 119), row_tombs=[(110, 110)]),
    # no filter at all: ts 99 is in front of t0, ts 120 is bucket 2 of 2,
    # ts 500 far behind
    _hand("outside_buckets", [5], [99, 100, 119, 120, 500],
          [_i([7, -3, 5, 11, 13])], [1, 1],
          [_cell(1, -3, -3, -3, -3, -3, 100, 100),
           _cell(1, 5, 5, 5, 5, 5, 119, 119)]),
    # bucket_ns 0: one bucket, t0 plays no part.  NaN counts, poisons the
    # sum, is first and last, and enters neither bound
    _hand("nan", [4], [1, 2, 3, 4], [_f([NAN, 2.0, 1.0, NAN])], [4],
          [_cell(4, NAN, 1.0, 2.0, NAN, NAN, 1, 4)],
          t0=10**6, bucket_ns=0, n_buckets=1),
    # only NaN: the bounds keep their start values although count is 2
    _hand("only_nan", [2], [100, 101], [_f([NAN, NAN])], [2],
          [_cell(2, NAN, INF, -INF, NAN, NAN, 100, 101)], n_buckets=1),
    # +0.0 first: both bounds keep +0.0
    _hand("zeros_plus_first", [3], [100, 101, 102], [_f([0.0, -0.0, 0.0])],
          [3], [_cell(3, 0.0, 0.0, 0.0, 0.0, 0.0, 100, 102)], n_buckets=1),
    # -0.0 first: both bounds keep -0.0
    _hand("zeros_minus_first", [2], [100, 101], [_f([-0.0, 0.0])], [2],
          [_cell(2, 0.0, NEG0, NEG0, NEG0, 0.0, 100, 101)], n_buckets=1),
    # (2^63 - 1) + 1 + (2^63 - 1) = 2^64 - 1, which is -1 as i64
    _hand("i64_sum_wraps", [3], [100, 101, 102],
          [_i([I64_MAX, 1, I64_MAX])], [3, 0],
          [_cell(3, -1, 1, I64_MAX, I64_MAX, I64_MAX, 100, 102), _E_I64]),
    # (2^63 + 5) + 3 + (2^64 - 1) = 2^64 + 2^63 + 7; a signed compare would
    # call 2^63 + 5 the minimum
    _hand("u64_above_2_63", [3], [100, 101, 102],
          [fr.Col(CT_U64, np.array([2**63 + 5, 3, 2**64 - 1], np.uint64))],
          [3, 0],
          [_cell(3, 2**63 + 7, 3, 2**64 - 1, 2**63 + 5, 2**64 - 1, 100, 102),
           _E_U64]),
    # the null cell at ts 102 is true but does not count; sum = true cells
    _hand("bool", [4], [100, 101, 102, 103],
          [fr.Col(CT_BOOL, np.array([1, 0, 1, 1], np.uint8),
                  np.array([1, 1, 0, 1], bool))], [4, 0],
          [_cell(3, 2, 0, 1, 1, 1, 100, 103), _E_BOOL]),
    # two series: (s0, b1) and (s1, b0) have no row
    _hand("empty_cells", [2, 1], [100, 101, 115], [_i([4, 6, 9])],
          [2, 0, 0, 1],
          [_cell(2, 10, 4, 6, 4, 6, 100, 101), _E_I64, _E_I64,
           _cell(1, 9, 9, 9, 9, 9, 115, 115)]),
    # nothing passes the predicate
    _hand("all_filtered", [3], [100, 105, 111], [_f([1.0, 2.0, 3.0])],
          [0, 0], [_E_F64, _E_F64], preds=[(0, "gt", 1000.0)]),
    # the predicate is on another column: rows 0 and 2 are kept
    _hand("predicate_on_other_column", [3], [100, 101, 102],
          [_f([1.5, 2.5, 4.0]), _i([1, 0, 1])], [2],
          [_cell(2, 5.5, 1.5, 4.0, 1.5, 4.0, 100, 102)],
          preds=[(1, "gt", 0)], n_buckets=1),
    # three series into one cell: ts 100 is shared by series 0 and 1 (first
    # = the lower series), ts 107 by series 1 and 2 (last = the higher)
    _hand("tie_across_series", [2, 2, 2], [100, 105, 100, 107, 103, 107],
          [_f([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])], [6],
          [_cell(6, 21.0, 1.0, 6.0, 1.0, 6.0, 100, 107)],
          n_buckets=1, per_series=False),
    # the same rows per series
    _hand("per_series_of_the_tie", [2, 2, 2], [100, 105, 100, 107, 103, 107],
          [_f([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])], [2, 2, 2],
          [_cell(2, 3.0, 1.0, 2.0, 1.0, 2.0, 100, 105),
           _cell(2, 7.0, 3.0, 4.0, 3.0, 4.0, 100, 107),
           _cell(2, 11.0, 5.0, 6.0, 5.0, 6.0, 103, 107)], n_buckets=1),
    # per_series 0 with an empty bucket and +0.0 / -0.0 across series: the
    # first row of the SET decides, here series 0's -0.0
    _hand("zeros_across_series", [1, 1], [100, 100], [_f([-0.0, 0.0])],
          [2, 0],
          [_cell(2, 0.0, NEG0, NEG0, NEG0, 0.0, 100, 100), _E_F64],
          per_series=False),
]


def hand_bits(ctype, name, v):
    """A hand-written value as the raw pattern the arrays hold."""
    if name in ("count", "first_ts", "last_ts"):
        return int(v)
    if isinstance(v, float):
        return fr.bits(CT_F64, v)
    return int(v) & M64   # ints, NEG0 and the 0 bits of an empty first/last


def check_against_hand(h, got):
    """Messages for every place where `got` (agg_ref's layout) differs from
    the hand-written cells of h."""
    bad = []
    ct = h.ac.case.cols[0].ctype
    if list(got["rows"]) != list(h.want["rows"]):
        bad.append(f"{h.name}: rows {got['rows']} != {h.want['rows']}")
    g = got["cols"][0]
    for i, cell in enumerate(h.want["cells"]):
        for n in NAMES:
            w = hand_bits(ct, n, cell[n])
            v = g[n][i]
            same = v == w
            if n == "sum" and ct == CT_F64:
                # hand sums are exact in any order; +0.0 == -0.0 here
                a, b = value_of(CT_F64, v), value_of(CT_F64, w)
                same = (math.isnan(a) and math.isnan(b)) or a == b
            if not same:
                bad.append(f"{h.name}: cell {i} {n} {v:#x} != {w:#x}")
    return bad


# ------------------------------------------------------------------- fuzz

def fuzz_case(seed):
    """filter_ref.fuzz_case(seed) with a random aggregate on top.  Columns,
    values, null patterns, column tombstones and series sizes are taken as
    they come.  The filter is reshaped so that a case usually keeps some
    rows but not all: at most two predicates, each keeping a tenth of the
    rows on its own; a time range, when there is one, that cuts at most a
    fifth off either end; and one more row tombstone in the middle.  The
    buckets either end inside the longest series (short series then leave
    cells empty) or run past its end (the last bucket is empty)."""
    r = np.random.default_rng(10_000 + seed)
    case = fr.fuzz_case(seed)
    k = 0
    while not case.cols or len(case.ts) < 16:
        k += 1
        case = fr.fuzz_case(100_000 + 1000 * seed + k)
    ts = np.asarray(case.ts, np.int64)
    lo, hi = int(ts.min()), int(ts.max())
    span = hi - lo + 1
    preds = []
    for p in case.preds[:2]:
        alone = case._replace(preds=[p], time_range=None, row_tombs=())
        if fr.filter_ref(alone).keep.sum() * 10 >= len(ts):
            preds.append(p)
    time_range = None
    if case.time_range is not None:
        time_range = (lo + int(span * r.uniform(0, 0.2)),
                      hi - int(span * r.uniform(0, 0.2)))
    mid = lo + int(span * r.uniform(0.3, 0.6))
    row_tombs = list(case.row_tombs) + [(mid, mid + span // 20)]
    case = case._replace(preds=preds, time_range=time_range,
                         row_tombs=row_tombs)
    per_series = bool(r.random() < 0.6)
    n_buckets = int(r.integers(2 if per_series else 3, 9))
    t0 = lo + int(r.integers(-2, max(span // 8, 1) + 1))
    if per_series and r.random() < 0.5:
        cover = span * r.uniform(0.3, 0.9)
    else:
        cover = span * n_buckets / (n_buckets - 1) * r.uniform(1.05, 1.5)
    bucket_ns = max(int(cover) // n_buckets, 1)
    if r.random() < 0.06:
        bucket_ns, n_buckets = 0, 1
    ncols = len(case.cols)
    naggs = int(r.integers(1, min(ncols, 8) + 1))
    aggs = []
    for c in r.choice(ncols, naggs, replace=False):
        names = tuple(n for n in NAMES if r.random() < 0.6)
        aggs.append((int(c), names))
    return AggCase(case, aggs, t0, bucket_ns, n_buckets, per_series)


FUZZ_SEEDS = range(50)


# --------------------------------------------------------- host check files

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(REPO, "tests", "cpu", "agg_check.cpp")
CHECK_INC = os.path.join(REPO, "cnosdb_amd", "csrc")


def bucket_probes():
    """(ts, t0, bucket_ns, n_buckets) around every rule, and at the int64
    extremes, where ts - t0 does not fit int64."""
    out = []
    for t0, bn, nb in [(100, 10, 2), (0, 1, 5), (-50, 7, 3), (100, 0, 1),
                       (I64_MAX, 1, 4), (I64_MIN, 1, 4), (I64_MIN, I64_MAX, 3),
                       (I64_MAX, I64_MAX, 1), (I64_MIN, I64_MAX, 2**31 - 1),
                       (-1, 2**62, 4), (fr.T0, 300 * 10**9, 12)]:
        pts = {I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX}
        for k in sorted({0, 1, 2, nb - 1, nb, nb + 1}):
            for d in (-1, 0, 1):
                v = t0 + k * bn + d
                if I64_MIN <= v <= I64_MAX:
                    pts.add(v)
        out += [(ts, t0, bn, nb) for ts in sorted(pts)]
    return out


def random_runs(n=300, seed=7):
    """(ctype, [(ts, bits, row, valid)]) runs of at most 40 rows: values of
    filter_ref's domains (NaN, both zeros, the integer extremes), rising
    timestamps with some ties, rising rows, some null cells."""
    r = np.random.default_rng(seed)
    runs = []
    for _ in range(n):
        ct = int(r.choice([CT_I64, CT_F64, CT_BOOL, CT_U64]))
        m = int(r.integers(0, 41))
        dom = fr._VALUES[ct]
        ts = I64_MIN + 5 if r.random() < 0.1 else int(r.integers(-50, 50))
        row = int(r.integers(0, 2**40))
        rows = []
        for _ in range(m):
            ts += int(r.integers(0, 3)) if r.random() < 0.3 else int(
                r.integers(1, 1000))
            row += int(r.integers(1, 200))
            x = dom[int(r.integers(0, len(dom)))]
            rows.append((ts, fr.bits(ct, x), row, bool(r.random() < 0.85)))
        runs.append((ct, rows))
    return runs


def hand_runs():
    """Every cell of the hand-written table as a run."""
    runs = []
    for h in HAND:
        case = h.ac.case
        c = case.cols[0]
        ev = fr.effective(c, np.asarray(case.ts, np.int64))
        for cell in cell_rows(h.ac)[1]:
            runs.append((c.ctype, [(int(case.ts[r]), fr.bits(c.ctype, c.val[r]),
                                    r, bool(ev[r])) for r in cell]))
    return runs


def write_cases_file(path):
    """The input of tests/cpu/agg_check.cpp (its header comment has the
    layout).  Every expectation comes from this module.  Returns (runs,
    bucket probes)."""
    runs = hand_runs() + random_runs()
    probes = bucket_probes()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(runs)))
        for ct, rows in runs:
            want = reduce_rows(ct, [(ts, b) for ts, b, _, v in rows if v])
            f.write(struct.pack("<iI", ct, len(rows)))
            for ts, b, row, v in rows:
                f.write(struct.pack("<qQqI", ts, b, row, int(v)))
            f.write(struct.pack("<qQQQQQqq", want["count"], want["sum"],
                                want["min"], want["max"], want["first"],
                                want["last"], want["first_ts"],
                                want["last_ts"]))
            f.write(struct.pack("<d", want["sum_abs"]))
        f.write(struct.pack("<I", len(probes)))
        for ts, t0, bn, nb in probes:
            b = bucket_of(ts, t0, bn, nb)
            f.write(struct.pack("<qqqiii", ts, t0, bn, nb,
                                int(b is not None), -1 if b is None else b))
    return len(runs), len(probes)


def run_host_check(workdir, sanitize=True):
    """Build tests/cpu/agg_check.cpp in `workdir` and run it over the case
    file.  Returns (finished process, runs, probes), or None without a
    compiler."""
    cxx = host_compiler()
    if cxx is None:
        return None
    exe = os.path.join(str(workdir), "agg_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g"] +
                   (SANITIZE if sanitize else []) +
                   ["-I", CHECK_INC, CHECK_SRC, "-o", exe], check=True)
    path = os.path.join(str(workdir), "agg_cases.bin")
    counts = write_cases_file(path)
    res = subprocess.run([exe, path], capture_output=True, text=True)
    return (res,) + counts
