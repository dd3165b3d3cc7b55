"""Host side of the column-group re-encode: page_of(CT_U64) (the i64
codec over the bit-cast values, codec/unsigned.rs:15-18) and the folding
of page statistics into prune_column_groups' tuples."""
import numpy as np
import pytest

import cnosdb_amd as gs
from oracle import pyoracle as orc

rng = np.random.default_rng(77)

U64_CASES = {
    "above_2_63": np.uint64(1 << 63) + rng.integers(0, 1 << 40, 300).astype(np.uint64),
    "both_sides": np.array([0, 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1, 5],
                           dtype=np.uint64),
    "small": rng.integers(0, 1000, 257).astype(np.uint64),
    "equal_step": np.uint64((1 << 63) - 50) + np.arange(100, dtype=np.uint64),
    "one": np.array([(1 << 64) - 1], dtype=np.uint64),
}


def _split(page):
    nb = int.from_bytes(page[0:4], "big")
    nrows = int.from_bytes(page[4:12], "big")
    return nrows, page[16:16 + nb], page[16 + nb:]


@pytest.mark.parametrize("name", sorted(U64_CASES))
def test_page_of_u64_all_valid(name):
    v = U64_CASES[name]
    page = gs.page_of(v, gs.CT_U64)
    assert page == gs.page_of(v.view(np.int64), gs.CT_I64)
    nrows, _, data = _split(page)
    assert nrows == v.size
    assert data == orc.encode_i64(v.view(np.int64))
    got = orc.decode_i64(data, nrows)
    assert got.view(np.uint64).tolist() == v.tolist()


@pytest.mark.parametrize("name", sorted(U64_CASES))
def test_page_of_u64_with_nulls(name):
    v = U64_CASES[name]
    valid = rng.random(v.size) > 0.3
    valid[0] = False
    page = gs.page_of(v, gs.CT_U64, valid)
    nrows, bitset, data = _split(page)
    assert nrows == v.size
    assert bitset == np.packbits(valid, bitorder="little").tobytes()
    assert data == orc.encode_i64(v[valid].view(np.int64))
    got = orc.decode_i64(data, nrows, valid).view(np.uint64)
    assert got[valid].tolist() == v[valid].tolist()
    assert not got[~valid].any()


def _info(dtype, rows):
    a = np.zeros(len(rows), dtype=[("len", "<i8"), ("null_count", "<i8"),
                                   ("min", dtype), ("max", dtype)])
    for i, (nulls, mn, mx) in enumerate(rows):
        a[i] = (100, nulls, mn, mx)
    return a


def test_fold_page_stats_per_page_and_ranges():
    DM = np.finfo(np.float64).max
    pages_t = [np.array([10, 20, 30]), np.array([40, 50]), np.array([60]),
               np.array([70, 80, 90, 100])]
    pages_v = [np.array([1.5, -2.0, 3.0]), np.array([np.nan, np.nan]),
               np.array([7.0]), np.array([-9.5, 0.25, 4.0, 4.0])]
    valid_v = [np.array([1, 1, 1], bool), np.array([0, 0], bool),  # all null
               np.array([1], bool), np.array([1, 0, 1, 1], bool)]
    ts_info = _info("<i8", [(0, t.min(), t.max()) for t in pages_t])
    rows = []
    for v, m in zip(pages_v, valid_v):
        if m.any():
            rows.append((int((~m).sum()), v[m].min(), v[m].max()))
        else:  # the reference loop's starting values
            rows.append((v.size, DM, -DM))
    val_info = _info("<f8", rows)

    per_page = gs.fold_page_stats(ts_info, val_info)
    assert len(per_page) == 4
    for p, st in enumerate(per_page):
        assert st[0] == pages_t[p].min() and st[1] == pages_t[p].max()
        if valid_v[p].any():
            assert st[2] == pages_v[p][valid_v[p]].min()
            assert st[3] == pages_v[p][valid_v[p]].max()
        else:
            assert st[2] is None and st[3] is None

    ranges = [(0, 2), (1, 2), (1, 4), (0, 4)]
    folded = gs.fold_page_stats(ts_info, val_info, ranges)
    for (p0, p1), st in zip(ranges, folded):
        t = np.concatenate(pages_t[p0:p1])
        v = np.concatenate(pages_v[p0:p1])[np.concatenate(valid_v[p0:p1])]
        assert st[0] == t.min() and st[1] == t.max()
        if v.size:
            assert (st[2], st[3]) == (v.min(), v.max())
        else:
            assert st[2] is None and st[3] is None

    # no value column: time only; the tuples feed prune_column_groups
    time_only = gs.fold_page_stats(ts_info)
    assert [st[2:] for st in time_only] == [(None, None)] * 4
    assert gs.prune_column_groups(time_only, time_range=(35, 65)) == \
        [False, True, True, False]
    # the all-null page has no stats, so a value predicate never drops it
    assert gs.prune_column_groups(per_page, value_pred=("gt", 5.0)) == \
        [False, True, True, False]


def test_fold_page_stats_integer_types():
    big = np.array([1, (1 << 63) + 5, 1 << 63], dtype=np.uint64)
    u_info = _info("<u8", [(0, big.min(), big.max()),
                           (3, np.iinfo(np.uint64).max, 0)])
    i_info = _info("<i8", [(0, -5, 9), (0, -(1 << 62), 1 << 62)])
    ts_info = _info("<i8", [(0, 1, 2), (0, 3, 4)])
    st = gs.fold_page_stats(ts_info, u_info, [(0, 2)])[0]
    assert st == (1, 4, 1, (1 << 63) + 5)
    st = gs.fold_page_stats(ts_info, i_info, [(0, 2)])[0]
    assert st == (1, 4, -(1 << 62), 1 << 62)
