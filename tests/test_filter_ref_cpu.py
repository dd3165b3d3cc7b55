"""tests/filter_ref.py, the expectation of the gs_filter_group tests, tied
down on the CPU: its cell verdicts to the hand-written truth table, its
tombstone and time-range terms to the oracle's restatement of the
reference (pyoracle.update_nullbits, pyoracle.time_span) on sorted
timestamps, its whole-set result to a case small enough to work out by
hand.  The last tests hold the host binding's constant conversion
(cnosdb_amd.pred_bits) to the same bits."""
import numpy as np
import pytest

import filter_ref as fr
from oracle import pyoracle as orc


def test_truth_table_is_complete():
    ops = set(fr.OP_CODE) - set(fr.NULL_TESTS)
    for ct in (fr.CT_I64, fr.CT_U64, fr.CT_F64, fr.CT_BOOL):
        rows = [t for t in fr.TRUTH if t[0] == ct]
        assert {t[1] for t in rows} == ops, ct
        for op in ops:  # each op is seen passing and failing
            assert {t[5] for t in rows if t[1] == op} == {True, False}, (ct, op)
    cts = {ct for ct, _ in fr.NULL_TEST_CELLS}
    assert cts == {fr.CT_I64, fr.CT_U64, fr.CT_F64, fr.CT_BOOL, fr.CT_STR}
    # nothing goes through a double: the table holds pairs a double merges
    assert any(t[0] == fr.CT_I64 and float(t[2]) == float(t[4])
               and t[2] != t[4] for t in fr.TRUTH)
    assert any(t[0] == fr.CT_U64 and float(t[2]) == float(t[4])
               and t[2] != t[4] for t in fr.TRUTH)


def test_cell_agrees_with_the_truth_table():
    cells = fr.truth_cells()
    assert len(cells) == 3 * len(fr.TRUTH) + 6 * len(fr.NULL_TEST_CELLS)
    wrong = [c for c in cells
             if fr.cell(c[1], c[0], c[2], c[3], c[4],
                        fr.STATES[c[5]][2]) != c[6]]
    assert wrong == []


def test_states_reach_filter_ref_as_effective_validity():
    """A null cell and a tombstoned cell behave alike in filter_ref: one
    column, three rows (valid, null, valid inside a deleted range)."""
    ts = fr.T0 + np.arange(3, dtype=np.int64)
    tomb = [(int(ts[2]), int(ts[2]))]
    for ct, op, a, b, x, verdict in fr.TRUTH:
        col = fr.Col(ct, np.array([x] * 3, dtype=fr.NP_DTYPE[ct]),
                     np.array([1, 0, 1], bool), tomb)
        pred = (0, op, a) if b is None else (0, op, a, b)
        res = fr.filter_ref(fr.Case("t", [3], ts, [col], [], [pred]))
        assert res.keep.tolist() == [verdict, False, False], (ct, op, a, x)
        res = fr.filter_ref(fr.Case("t", [3], ts, [col], [],
                                    [(0, "is_null")]))
        assert res.keep.tolist() == [False, True, True]
        assert res.cols[0][1].tolist() == [0, 0]
        assert not res.cols[0][0].any()  # null cells come out as zero bytes


@pytest.mark.parametrize("seed", range(8))
def test_range_terms_against_the_oracle(seed):
    """On sorted timestamps the closed-range test is update_nullbits and the
    time range is time_span."""
    r = np.random.default_rng(seed)
    n = int(r.integers(1, 400))
    ts = fr.T0 + np.cumsum(r.integers(1, 5, n)).astype(np.int64)
    ranges = []
    for _ in range(int(r.integers(0, 6))):
        a, b = sorted(int(v) for v in
                      r.integers(int(ts[0]) - 3, int(ts[-1]) + 4, 2))
        ranges.append((a, b))
    # ends exactly on rows, and strictly between two rows
    ranges.append((int(ts[n // 2]), int(ts[-1])))
    if n > 1 and ts[1] - ts[0] > 1:
        ranges.append((int(ts[0]) + 1, int(ts[1]) - 1))
    valid = r.random(n) >= 0.2
    want = orc.update_nullbits(ts, ranges, valid)
    got = fr.effective(fr.Col(fr.CT_I64, np.zeros(n, np.int64), valid,
                              ranges), ts)
    assert got.tolist() == want.tolist()
    assert (fr.in_ranges(ts, fr.normalise(ranges)).tolist()
            == fr.in_ranges(ts, ranges).tolist())
    lo, hi = sorted(int(v) for v in
                    r.integers(int(ts[0]) - 3, int(ts[-1]) + 4, 2))
    s, c = orc.time_span(ts, lo, hi)
    res = fr.filter_ref(fr.Case("t", [n], ts, [fr.Col(fr.CT_I64,
                                np.arange(n, dtype=np.int64))], [], [],
                                (lo, hi)))
    assert np.flatnonzero(res.keep).tolist() == list(range(s, s + c))


def test_whole_set_by_hand():
    """Two groups, an i64 and a string column, a row tombstone, a column
    tombstone and two predicates, worked out by hand."""
    ts = np.array([10, 20, 30, 40, 10, 20, 30], np.int64)
    col = fr.Col(fr.CT_I64, np.array([5, 6, 7, 8, 9, 1, 7], np.int64),
                 np.array([1, 1, 0, 1, 1, 1, 1], bool), [(40, 40)])
    s = fr.StrCol([b"a", b"bb", b"ccc", b"dddd", b"e", b"ff", b"ggg"],
                  np.array([1, 0, 1, 1, 1, 1, 1], bool), [(30, 35)])
    case = fr.Case("hand", [4, 3], ts, [col], [s],
                   [(0, "ge", 5), (1, "is_not_null")], (10, 40),
                   [(20, 20)])
    res = fr.filter_ref(case)
    # rows 1 and 5 fall to the row tombstone; 2 is null, 3 is tombstoned in
    # the i64 column; 6's string is tombstoned; rows 0 and 4 remain
    assert res.keep.tolist() == [True, False, False, False, True, False,
                                 False]
    assert res.out_rows == 2 and res.offsets.tolist() == [0, 1, 2]
    assert res.ts.tolist() == [10, 10]
    assert res.cols[0][0].view(np.int64).tolist() == [5, 9]
    assert res.strs[0][0].tolist() == [0, 1, 2]
    assert bytes(res.strs[0][1]) == b"ae"


# ------------------------------------------------ the host binding's part

def test_pred_bits_matches_the_reference_bits():
    import cnosdb_amd as gs
    for ct, op, a, b, x, _ in fr.TRUTH:
        for v in (a, b, x):
            if v is not None:
                assert gs.pred_bits(ct, v) == fr.bits(ct, v), (ct, v)
    assert gs.pred_bits(gs.CT_I64, -1) == 2**64 - 1
    assert gs.pred_bits(gs.CT_F64, 3) == fr.bits(fr.CT_F64, 3.0)
    assert gs.pred_bits(gs.CT_BOOL, True) == 1
    assert gs.pred_bits(gs.CT_I64, np.int64(-2**63)) == 2**63
    assert gs.FILTER_OPS == fr.OP_CODE


@pytest.mark.parametrize("ctype,value,exc", [
    (1, 3.5, TypeError),           # float on an i64 column
    (1, 3.0, TypeError),           # even an integral one
    (4, 1.0, TypeError),
    (3, 0.0, TypeError),
    (4, -1, ValueError),           # negative on u64
    (1, 2**63, OverflowError),
    (1, -2**63 - 1, OverflowError),
    (4, 2**64, OverflowError),
    (3, 2, ValueError),
    (2, 2**53 + 1, ValueError),    # an int a double cannot hold
    (2, True, TypeError),
    (1, True, TypeError),
    (1, "5", TypeError),
    (5, 1, ValueError),            # strings take no constants
])
def test_pred_bits_refuses_what_does_not_fit(ctype, value, exc):
    import cnosdb_amd as gs
    with pytest.raises(exc):
        gs.pred_bits(ctype, value)
