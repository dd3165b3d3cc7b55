"""What gs_filter_group must compute, restated in numpy from the semantics
in include/cnosdb_gs.h, and the designed cases of its tests.

The restatement knows rows only: no tiles, no segments, no device code.
Integer cells are compared as Python ints (object arrays), so no compare
can pass through a double or wrap; f64 cells with numpy's IEEE operators.
A deleted range is the closed interval it says, tested on every row for
itself, whatever the order of the timestamps or of the list.

TRUTH is hand-written: every verdict in it was decided by a person from the
header's rules, not produced by any code.  tests/test_filter_ref_cpu.py
holds `cell` to it; the host check (tests/cpu/filter_check.cpp) and the
device then have to agree with both.

Built from numpy alone.  Not a test module and not a conftest."""
import math
import os
import struct
import subprocess
from collections import namedtuple

import numpy as np

from str_corpus import SANITIZE, host_compiler

CT_I64, CT_F64, CT_BOOL, CT_U64, CT_STR = 1, 2, 3, 4, 5
OP_CODE = {"gt": 1, "ge": 2, "lt": 3, "le": 4, "eq": 5, "ne": 6,
           "between": 7, "is_null": 8, "is_not_null": 9}
NULL_TESTS = ("is_null", "is_not_null")
NP_DTYPE = {CT_I64: np.int64, CT_F64: np.float64, CT_BOOL: np.uint8,
            CT_U64: np.uint64}
I64_MIN, I64_MAX = -2**63, 2**63 - 1
T0 = 1_700_000_000_000_000_000
NAN, INF = float("nan"), float("inf")

# ---------------------------------------------------------------- the rules


def _cells(ctype, values):
    """Values of one column as the compare sees them: Python ints for the
    integer types and bool, float64 for f64."""
    if ctype == CT_F64:
        return np.asarray(values, dtype=np.float64)
    out = np.empty(len(values), dtype=object)
    out[:] = [int(v) for v in values]
    return out


def _compare(op, ctype, a, b, x):
    """The verdict of a comparison op over the cells x (as _cells gives
    them), every cell taken as valid."""
    if ctype == CT_F64:
        a, b = np.float64(a), np.float64(0.0 if b is None else b)
    else:
        a, b = int(a), int(0 if b is None else b)
    with np.errstate(invalid="ignore"):
        if op == "gt":
            r = x > a
        elif op == "ge":
            r = x >= a
        elif op == "lt":
            r = x < a
        elif op == "le":
            r = x <= a
        elif op == "eq":
            r = x == a
        elif op == "ne":
            r = x != a
        elif op == "between":
            r = (x >= a) & (x <= b)
        else:
            raise ValueError(op)
    return np.asarray(r, dtype=bool)


def cell(op, ctype, a, b, x, valid):
    """Verdict of one cell; valid is its EFFECTIVE validity.  The null tests
    never look at x; a comparison on a null cell fails."""
    if op == "is_null":
        return not valid
    if op == "is_not_null":
        return bool(valid)
    if not valid:
        return False
    return bool(_compare(op, ctype, a, b, _cells(ctype, [x]))[0])


def in_ranges(ts, ranges):
    """Row r lies in a range iff min_ts <= ts[r] <= max_ts: every range for
    itself, a range with min > max matching nothing."""
    ts = np.asarray(ts, dtype=np.int64)
    hit = np.zeros(ts.size, dtype=bool)
    for mn, mx in ranges:
        hit |= (ts >= mn) & (ts <= mx)
    return hit


def normalise(ranges):
    """Normal form of a range list, in unbounded ints: empty ranges dropped,
    sorted, overlapping and touching closed ranges merged."""
    out = []
    for mn, mx in sorted((int(a), int(b)) for a, b in ranges if a <= b):
        if out and mn <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], mx)
        else:
            out.append([mn, mx])
    return [tuple(r) for r in out]


def bits(ctype, v):
    """A constant or cell value as raw 64 bits in the column's type."""
    if ctype == CT_F64:
        return struct.unpack("<Q", struct.pack("<d", float(v)))[0]
    return int(v) & (2**64 - 1)


# one fixed-width column / one string column of a case
Col = namedtuple("Col", "ctype val valid tombs project out_valid",
                 defaults=(None, (), True, True))
StrCol = namedtuple("StrCol", "strings valid tombs project out_valid",
                    defaults=(None, (), True, True))
Case = namedtuple("Case", "name sizes ts cols strs preds time_range "
                          "row_tombs", defaults=((), (), None, ()))
Result = namedtuple("Result", "keep out_rows offsets ts cols strs")


def effective(col, ts):
    n = len(ts)
    v = np.ones(n, bool) if col.valid is None else np.asarray(col.valid, bool)
    return v & ~in_ranges(ts, col.tombs)


def filter_ref(case):
    """Result of gs_filter_group over `case`.  cols[c] / strs[s] of the
    result are None for a column that is not projected; else (value bytes
    as uint8, validity uint8) and (offsets int64, bytes uint8, validity
    uint8)."""
    ts = np.asarray(case.ts, dtype=np.int64)
    n = ts.size
    lo, hi = case.time_range if case.time_range else (I64_MIN, I64_MAX)
    keep = (ts >= lo) & (ts <= hi) & ~in_ranges(ts, case.row_tombs)
    allc = list(case.cols) + list(case.strs)
    eff = [effective(c, ts) for c in allc]
    for pred in case.preds:
        col, op = pred[0], pred[1]
        ev = eff[col]
        if op == "is_null":
            keep &= ~ev
        elif op == "is_not_null":
            keep &= ev
        else:
            c = case.cols[col]
            a = pred[2]
            b = pred[3] if len(pred) > 3 else None
            keep &= ev & _compare(op, c.ctype, a, b, _cells(c.ctype, c.val))
    cols = []
    for c, ev in zip(case.cols, eff):
        if not c.project:
            cols.append(None)
            continue
        v = np.asarray(c.val, dtype=NP_DTYPE[c.ctype]).copy()
        v[~ev] = 0
        cols.append((np.ascontiguousarray(v[keep]).view(np.uint8),
                     ev[keep].astype(np.uint8)))
    strs = []
    for c, ev in zip(case.strs, eff[len(case.cols):]):
        if not c.project:
            strs.append(None)
            continue
        cells = [c.strings[r] if ev[r] else b"" for r in np.flatnonzero(keep)]
        off = np.zeros(len(cells) + 1, np.int64)
        np.cumsum([len(s) for s in cells], out=off[1:])
        strs.append((off, np.frombuffer(b"".join(cells), np.uint8),
                     ev[keep].astype(np.uint8)))
    starts = np.concatenate([[0], np.cumsum(case.sizes)]).astype(np.int64)
    assert starts[-1] == n
    prefix = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return Result(keep, int(keep.sum()), prefix[starts], ts[keep], cols, strs)


# ------------------------------------------------------- the truth table
# (ctype, op, a, b, x, verdict of a VALID cell).  A null cell, and a valid
# cell whose timestamp lies in one of its column's deleted ranges, fails
# every comparison, passes is_null and fails is_not_null: see STATES.

P53 = 2**53
TRUTH = [
    # ---- i64: signed, exact beyond 2^53
    (CT_I64, "gt", 4, None, 5, True),
    (CT_I64, "gt", 4, None, 4, False),
    (CT_I64, "gt", 0, None, -1, False),      # unsigned would say True
    (CT_I64, "gt", P53, None, P53 + 1, True),    # equal as doubles
    (CT_I64, "gt", P53, None, P53, False),
    (CT_I64, "gt", P53 + 1, None, P53 + 1, False),
    (CT_I64, "gt", P53 + 1, None, P53 + 2, True),
    (CT_I64, "ge", 4, None, 4, True),
    (CT_I64, "ge", 4, None, 3, False),
    (CT_I64, "ge", P53 + 1, None, P53, False),   # a double says True
    (CT_I64, "ge", P53 + 1, None, P53 + 1, True),
    (CT_I64, "lt", I64_MIN + 1, None, I64_MIN, True),
    (CT_I64, "lt", 4, None, 4, False),
    (CT_I64, "lt", P53 + 1, None, P53, True),    # a double says False
    (CT_I64, "lt", -1, None, I64_MAX, False),
    (CT_I64, "le", 4, None, 4, True),
    (CT_I64, "le", 4, None, 5, False),
    (CT_I64, "le", P53, None, P53 + 1, False),   # a double says True
    (CT_I64, "le", I64_MAX, None, I64_MAX, True),
    (CT_I64, "eq", P53 + 1, None, P53 + 1, True),
    (CT_I64, "eq", P53 + 1, None, P53, False),   # a double says True
    (CT_I64, "eq", -1, None, -1, True),
    (CT_I64, "eq", I64_MIN, None, I64_MAX, False),
    (CT_I64, "ne", P53 + 1, None, P53, True),    # a double says False
    (CT_I64, "ne", 7, None, 7, False),
    (CT_I64, "between", 5, 9, 5, True),
    (CT_I64, "between", 5, 9, 4, False),
    (CT_I64, "between", 5, 9, 9, True),
    (CT_I64, "between", 5, 9, 10, False),
    (CT_I64, "between", -9, -1, -5, True),
    (CT_I64, "between", P53 + 1, P53 + 1, P53 + 1, True),
    (CT_I64, "between", P53 + 1, P53 + 1, P53, False),
    (CT_I64, "between", P53 + 1, P53 + 1, P53 + 2, False),
    (CT_I64, "between", 9, 5, 7, False),         # empty interval
    # ---- u64: unsigned, exact around 2^63 and at 2^64 - 1
    (CT_U64, "gt", 2**63 - 1, None, 2**63, True),    # signed would say False
    (CT_U64, "gt", 2**63, None, 2**63, False),
    (CT_U64, "gt", 2**63, None, 2**64 - 1, True),
    (CT_U64, "gt", 2**64 - 1, None, 2**64 - 1, False),
    (CT_U64, "gt", 2**64 - 1, None, 0, False),
    (CT_U64, "ge", 2**63, None, 2**63, True),
    (CT_U64, "ge", 2**63, None, 2**63 - 1, False),
    (CT_U64, "ge", 2**64 - 1, None, 2**64 - 2, False),  # equal as doubles
    (CT_U64, "lt", 2**63, None, 2**63 - 1, True),
    (CT_U64, "lt", 2**63, None, 2**64 - 1, False),
    (CT_U64, "lt", 2**64 - 1, None, 2**64 - 2, True),
    (CT_U64, "le", 2**63 - 1, None, 2**63, False),
    (CT_U64, "le", 2**64 - 1, None, 2**64 - 1, True),
    (CT_U64, "le", 0, None, 0, True),
    (CT_U64, "eq", 2**64 - 1, None, 2**64 - 1, True),
    (CT_U64, "eq", 2**64 - 1, None, 2**64 - 2, False),
    (CT_U64, "eq", 2**63, None, 2**63 + 1, False),
    (CT_U64, "ne", 2**63, None, 2**63 + 1, True),
    (CT_U64, "ne", 2**63, None, 2**63, False),
    (CT_U64, "between", 2**63 - 1, 2**63 + 1, 2**63, True),
    (CT_U64, "between", 2**63 - 1, 2**63 + 1, 2**63 + 2, False),
    (CT_U64, "between", 2**63 - 1, 2**63 + 1, 0, False),
    (CT_U64, "between", 2**63, 2**64 - 1, 2**64 - 1, True),
    (CT_U64, "between", 0, 2**63 - 1, 2**63, False),
    # ---- f64: the IEEE operators
    (CT_F64, "gt", 90.0, None, 90.5, True),
    (CT_F64, "gt", 90.0, None, 90.0, False),
    (CT_F64, "gt", 90.0, None, NAN, False),
    (CT_F64, "gt", 1e308, None, INF, True),
    (CT_F64, "gt", 0.0, None, -0.0, False),
    (CT_F64, "gt", -0.0, None, 0.0, False),
    (CT_F64, "gt", NAN, None, 1.0, False),
    (CT_F64, "ge", 0.0, None, -0.0, True),
    (CT_F64, "ge", 90.0, None, NAN, False),
    (CT_F64, "ge", INF, None, INF, True),
    (CT_F64, "ge", 3.5, None, 3.0, False),
    (CT_F64, "lt", -1e308, None, -INF, True),
    (CT_F64, "lt", 0.0, None, -0.0, False),
    (CT_F64, "lt", 90.0, None, NAN, False),
    (CT_F64, "lt", INF, None, INF, False),
    (CT_F64, "le", -0.0, None, 0.0, True),
    (CT_F64, "le", 90.0, None, NAN, False),
    (CT_F64, "le", -INF, None, -INF, True),
    (CT_F64, "le", 5.0, None, 5.000000000000001, False),
    (CT_F64, "eq", 0.0, None, -0.0, True),
    (CT_F64, "eq", NAN, None, NAN, False),
    (CT_F64, "eq", INF, None, INF, True),
    (CT_F64, "eq", INF, None, -INF, False),
    (CT_F64, "eq", 0.1, None, 0.1, True),
    (CT_F64, "ne", NAN, None, NAN, True),
    (CT_F64, "ne", 1.0, None, NAN, True),
    (CT_F64, "ne", NAN, None, 1.0, True),
    (CT_F64, "ne", 0.0, None, -0.0, False),
    (CT_F64, "ne", INF, None, INF, False),
    (CT_F64, "ne", 1.0, None, 2.0, True),
    (CT_F64, "between", -INF, INF, 0.0, True),
    (CT_F64, "between", -INF, INF, NAN, False),
    (CT_F64, "between", 0.0, INF, INF, True),
    (CT_F64, "between", 0.0, 1.0, -0.0, True),
    (CT_F64, "between", -1.0, -0.0, 0.0, True),
    (CT_F64, "between", 0.0, NAN, 0.0, False),
    (CT_F64, "between", 1.0, 2.0, 2.5, False),
    # ---- bool: 0/1
    (CT_BOOL, "eq", 1, None, 1, True),
    (CT_BOOL, "eq", 1, None, 0, False),
    (CT_BOOL, "eq", 0, None, 0, True),
    (CT_BOOL, "ne", 0, None, 1, True),
    (CT_BOOL, "ne", 1, None, 1, False),
    (CT_BOOL, "gt", 0, None, 1, True),
    (CT_BOOL, "gt", 0, None, 0, False),
    (CT_BOOL, "ge", 1, None, 0, False),
    (CT_BOOL, "ge", 1, None, 1, True),
    (CT_BOOL, "lt", 1, None, 0, True),
    (CT_BOOL, "lt", 1, None, 1, False),
    (CT_BOOL, "le", 0, None, 1, False),
    (CT_BOOL, "le", 0, None, 0, True),
    (CT_BOOL, "between", 0, 1, 1, True),
    (CT_BOOL, "between", 1, 1, 0, False),
]
# the two null tests, on every fixed-width type and on strings: (ctype, x)
NULL_TEST_CELLS = [(CT_I64, -3), (CT_U64, 2**64 - 1), (CT_F64, NAN),
                   (CT_F64, 1.5), (CT_BOOL, 1), (CT_BOOL, 0),
                   (CT_STR, b"abc"), (CT_STR, b"")]
# state of a cell -> (raw validity, timestamp in a deleted range of its
# column, effective validity)
STATES = {"valid": (1, False, True), "null": (0, False, False),
          "tomb": (1, True, False)}


def truth_verdict(op, verdict_valid, state):
    """The hand-written rule for the three states of a cell."""
    effective_valid = STATES[state][2]
    if op == "is_null":
        return not effective_valid
    if op == "is_not_null":
        return effective_valid
    return verdict_valid if effective_valid else False


def truth_cells():
    """Every (ctype, op, a, b, x, state, verdict) of the table."""
    out = []
    for ct, op, a, b, x, v in TRUTH:
        for st in STATES:
            out.append((ct, op, a, b, x, st, truth_verdict(op, v, st)))
    for ct, x in NULL_TEST_CELLS:
        for op in NULL_TESTS:
            for st in STATES:
                out.append((ct, op, 0, None, x, st,
                            truth_verdict(op, None, st)))
    return out


# ------------------------------------------------------ designed range lists

def range_lists():
    """(name, list) for the normal form and the membership search."""
    r = np.random.default_rng(65)
    pts = r.permutation(np.arange(0, 65 * 10, 10))
    shuffled = [(int(p), int(p) + int(r.integers(0, 14))) for p in pts]
    return [
        ("empty", []),
        ("inverted", [(5, 4)]),
        ("inverted_among", [(10, 20), (9, 3), (30, 40), (I64_MAX, I64_MIN)]),
        ("single", [(7, 7)]),
        ("duplicate", [(3, 9), (3, 9), (3, 9)]),
        ("nested", [(0, 100), (10, 20), (30, 99), (100, 100)]),
        ("touching", [(1, 5), (6, 9)]),
        ("gap_of_one", [(1, 5), (7, 9)]),
        ("overlap_unsorted", [(50, 60), (10, 30), (25, 55), (70, 80)]),
        ("min_ended", [(I64_MIN, I64_MIN), (I64_MIN + 1, -5), (I64_MIN, 0)]),
        ("max_ended", [(I64_MAX, I64_MAX), (I64_MAX - 1, I64_MAX - 1),
                       (5, I64_MAX), (I64_MAX - 9, I64_MAX)]),
        ("whole_line", [(I64_MIN, I64_MAX), (3, 4)]),
        ("touching_at_max", [(0, I64_MAX - 1), (I64_MAX, I64_MAX)]),
        ("shuffled65", shuffled),
    ]


def probes(ranges):
    """Timestamps around every endpoint of the list, and the line's ends."""
    p = {I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX}
    for mn, mx in ranges:
        for e in (mn, mx):
            p.update(v for v in (e - 1, e, e + 1) if I64_MIN <= v <= I64_MAX)
    return sorted(p)


# --------------------------------------------------------- host check files

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(REPO, "tests", "cpu", "filter_check.cpp")
CHECK_INC = os.path.join(REPO, "cnosdb_amd", "csrc")


def write_cases_file(path):
    """The input of tests/cpu/filter_check.cpp (its header comment has the
    layout).  Every expectation comes from this module: the verdict of a
    cell from `cell`, the normal form from `normalise`, membership from
    `in_ranges` over the list AS GIVEN.  Returns (cells, lists, probes)."""
    cells = [c for c in truth_cells() if c[0] != CT_STR]
    lists = range_lists()
    nprobe = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cells)))
        for ct, op, a, b, x, st, _ in cells:
            ev = STATES[st][2]
            f.write(struct.pack("<iiQQQII", OP_CODE[op], ct, bits(ct, a),
                                bits(ct, 0 if b is None else b), bits(ct, x),
                                int(ev), int(cell(op, ct, a, b, x, ev))))
        f.write(struct.pack("<I", len(lists)))
        for name, lst in lists:
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm)
            f.write(struct.pack("<I", len(lst)))
            for mn, mx in lst:
                f.write(struct.pack("<qq", mn, mx))
            norm = normalise(lst)
            f.write(struct.pack("<I", len(norm)))
            for mn, mx in norm:
                f.write(struct.pack("<qq", mn, mx))
            ps = probes(lst)
            hit = in_ranges(np.array(ps, np.int64), lst)
            f.write(struct.pack("<I", len(ps)))
            for t, h in zip(ps, hit):
                f.write(struct.pack("<qI", t, int(h)))
            nprobe += len(ps)
    return len(cells), len(lists), nprobe


def run_host_check(workdir, sanitize=True):
    """Build tests/cpu/filter_check.cpp in `workdir` and run it over the
    case file.  Returns (finished process, cells, lists, probes), or None
    without a compiler."""
    cxx = host_compiler()
    if cxx is None:
        return None
    exe = os.path.join(str(workdir), "filter_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g"] +
                   (SANITIZE if sanitize else []) +
                   ["-I", CHECK_INC, CHECK_SRC, "-o", exe], check=True)
    path = os.path.join(str(workdir), "filter_cases.bin")
    counts = write_cases_file(path)
    res = subprocess.run([exe, path], capture_output=True, text=True)
    return (res,) + counts


# ------------------------------------------------------------ device cases

def group_ts(sizes, step=1_000_000_000):
    """Strictly increasing timestamps inside every group; the groups overlap
    in time, as series do."""
    return np.concatenate(
        [T0 + np.arange(n, dtype=np.int64) * step for n in sizes]
        + [np.zeros(0, np.int64)])


def edge_sizes(tile):
    """Group sizes around the wave (64), the wave segment (tile / 4) and
    the tile: four groups inside one tile, one group over three tiles."""
    seg = tile // 4
    return [1, 63, 64, 65, seg - 1, seg, seg + 1, tile - 1, tile, tile + 1,
            2 * tile + 1, 5, 6, 7, 8, 3 * tile + 17, 100]


_VALUES = {
    CT_I64: [-5, -1, 0, 1, 3, 5, P53, P53 + 1, I64_MIN, I64_MAX],
    CT_U64: [0, 1, 3, 5, 2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1],
    CT_F64: [-5.5, -0.0, 0.0, 1.0, 3.5, 90.5, NAN, INF, -INF],
    CT_BOOL: [0, 1],
}
_STR_LENS = (0, 1, 7, 8, 9, 40)


def _rand_ranges(r, ts, n):
    out = []
    lo, hi = int(ts.min()), int(ts.max())
    for _ in range(n):
        a, b = sorted(int(v) for v in r.integers(lo - 2, hi + 3, 2))
        if r.random() < 0.7:
            b = a + int(r.integers(0, 3))   # a short range
        if r.random() < 0.1:
            a, b = b + 1, a                 # inverted: matches nothing
        out.append((a, b))
    return out


def fuzz_case(seed, max_rows=20000):
    """One seeded set: 1-6 columns of random types, independent null
    patterns, 0-4 predicates, random ranges and tombstones."""
    r = np.random.default_rng(seed)
    nrows = int(math.exp(r.uniform(0.0, math.log(max_rows))))
    ngroups = int(r.integers(1, min(nrows, 12) + 1))
    cuts = np.sort(r.integers(0, nrows + 1, ngroups - 1))
    sizes = np.diff(np.concatenate([[0], cuts, [nrows]])).astype(int).tolist()
    ts = group_ts(sizes, step=int(r.integers(1, 4)))
    ncols = int(r.integers(1, 7))
    cols, strs = [], []
    for _ in range(ncols):
        ct = int(r.choice([CT_I64, CT_F64, CT_BOOL, CT_U64, CT_STR]))
        rate = float(r.choice([0.0, 0.1, 0.5, 1.0]))
        valid = None if r.random() < 0.25 else r.random(nrows) >= rate
        tombs = _rand_ranges(r, ts, int(r.integers(0, 4)))
        project, out_valid = bool(r.random() < 0.8), bool(r.random() < 0.8)
        if ct == CT_STR:
            lens = r.choice(_STR_LENS, nrows)
            strings = [bytes(r.integers(0x21, 0x7f, n, dtype=np.uint8))
                       for n in lens]
            strs.append(StrCol(strings, valid, tombs, project, out_valid))
        else:
            pick = r.integers(0, len(_VALUES[ct]), nrows)
            val = np.array(_VALUES[ct], dtype=NP_DTYPE[ct])[pick]
            cols.append(Col(ct, val, valid, tombs, project, out_valid))
    preds = []
    for _ in range(int(r.integers(0, 5))):
        c = int(r.integers(0, ncols))
        if c >= len(cols) or r.random() < 0.2:
            preds.append((c, str(r.choice(NULL_TESTS))))
            continue
        dom = _VALUES[cols[c].ctype]
        op = str(r.choice(["gt", "ge", "lt", "le", "eq", "ne", "between"]))
        a = dom[int(r.integers(0, len(dom)))]
        b = dom[int(r.integers(0, len(dom)))]
        preds.append((c, op, a, b) if op == "between" else (c, op, a))
    time_range = None
    if r.random() < 0.4:
        time_range = tuple(sorted(
            int(v) for v in r.integers(int(ts.min()) - 1, int(ts.max()) + 2,
                                       2)))
    row_tombs = _rand_ranges(r, ts, int(r.integers(0, 4)))
    return Case(f"fuzz{seed}", sizes, ts, cols, strs, preds, time_range,
                row_tombs)
