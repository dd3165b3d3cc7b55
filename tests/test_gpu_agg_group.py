"""gs_agg_group on the device: the keep rule of gs_filter_group reduced
straight into (series, bucket) cells.  Every cell of every requested array
is compared with tests/agg_ref.py: bit for bit, except the f64 sum, which is
held to |got - fsum| <= n * 2^-53 * sum|x| per cell (the bound of any
summation order of the cell's n values).  Output arrays start poisoned, so a
cell the call does not write fails the comparison."""
import itertools

import numpy as np
import pytest
import torch

import agg_ref as ar
import cnosdb_amd as gs
import filter_ref as fr

pytestmark = pytest.mark.gpu

GS_ERR, GS_ERR_FORMAT = -1, -3
POISON = 0xA5
WIDTH = {fr.CT_I64: 8, fr.CT_F64: 8, fr.CT_U64: 8, fr.CT_BOOL: 1}


@pytest.fixture(scope="module")
def engine():
    e = gs.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def tile():
    return gs.filter_tile()


# --------------------------------------------------------------- the runner

def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a writable copy


def _poison(nbytes):
    return torch.full((max(nbytes, 1),), POISON, dtype=torch.uint8,
                      device="cuda")


class _Dev:
    """A case's device inputs; the set is a raw set of the case's series
    unless one is given."""

    def __init__(self, engine, ac, gset=None, nseries=None):
        case = ac.case
        n = self.n = len(case.ts)
        sizes = ac.series if ac.series is not None else case.sizes
        self.nseries = nseries if gset is not None else len(sizes)
        self.gset = gset or engine.raw_set(np.array(sizes, np.int64))
        self.own_set = gset is None
        self.ts = _dev(np.asarray(case.ts, np.int64)) if n else _poison(8)
        self.cols, self.strs = [], []
        for c in case.cols:
            v = np.asarray(c.val, dtype=fr.NP_DTYPE[c.ctype])
            self.cols.append((
                c.ctype, _dev(v.view(np.uint8)) if n else _poison(8),
                None if c.valid is None else _dev(
                    np.asarray(c.valid, np.uint8)) if n else _poison(1),
                list(c.tombs)))
        for s in case.strs:
            off = np.zeros(n + 1, np.int64)
            np.cumsum([len(x) for x in s.strings], out=off[1:])
            data = np.frombuffer(b"".join(s.strings) + b"\0", np.uint8)
            self.strs.append((
                (_dev(off), _dev(data),
                 None if s.valid is None else _dev(
                     np.asarray(s.valid, np.uint8)) if n else _poison(1)),
                list(s.tombs), None))

    def call(self, engine, ac, aggs=None, per_series=None, want_rows=True):
        """Run the case; returns (rows per cell or None, per aggregated
        column {name: uint64 array over the cells})."""
        case = ac.case
        aggs = ac.aggs if aggs is None else aggs
        per_series = ac.per_series if per_series is None else per_series
        ncell = (self.nseries if per_series else 1) * ac.n_buckets
        outs = [(col, {n: _poison(ncell * 8) for n in names})
                for col, names in aggs]
        d_rows = _poison(ncell * 8) if want_rows else None
        engine.agg_group(self.gset, self.ts, self.cols, list(case.preds),
                         outs, ac.t0, ac.bucket_ns, ac.n_buckets, per_series,
                         self.strs, case.time_range, list(case.row_tombs),
                         d_rows=d_rows)
        view = lambda t: t.cpu().numpy()[:ncell * 8].view(np.uint64)  # noqa
        return (None if d_rows is None else view(d_rows),
                [{n: view(t) for n, t in want.items()} for _, want in outs])

    def free(self):
        if self.own_set:
            self.gset.free()


def _signed(v):
    return v - 2**64 if v >= 2**63 else v


def _check(ac, got_rows, got_cols, aggs=None, per_series=None, ref=None):
    """Hold device arrays to agg_ref: every requested name of every cell."""
    aggs = ac.aggs if aggs is None else aggs
    if per_series is not None:
        ac = ac._replace(per_series=per_series)
    ac = ac._replace(aggs=[(c, ar.NAMES) for c, _ in aggs])
    ref = ref or ar.agg_ref(ac)
    name = ac.case.name
    if got_rows is not None:
        assert got_rows.tolist() == ref["rows"], name + " rows"
    assert len(got_cols) == len(aggs)
    for (col, names), got, want in zip(aggs, got_cols, ref["cols"]):
        ct = ac.case.cols[col].ctype
        assert set(got) == set(names)
        for n in names:
            g = [int(x) for x in got[n]]
            assert len(g) == len(want[n]), (name, col, n)
            if n == "sum":
                for i, (a, b) in enumerate(zip(g, want[n])):
                    assert ar.sum_within(ct, a, b, want["count"][i],
                                         want["sum_abs"][i]), \
                        (name, col, i, hex(a), hex(b))
                continue
            if n in ("count", "first_ts", "last_ts"):
                g = [_signed(x) for x in g]
            assert g == want[n], (name, col, n)
    return ref


def _run(engine, ac, **kw):
    d = _Dev(engine, ac)
    try:
        rows, cols = d.call(engine, ac, **kw)
        return _check(ac, rows, cols, kw.get("aggs"), kw.get("per_series"))
    finally:
        d.free()


# ------------------------------------------------------ the hand-written table

@pytest.mark.parametrize("h", ar.HAND, ids=lambda h: h.name)
def test_hand_table_on_device(engine, h):
    """Held to the hand-written cells first, to agg_ref second; then the
    other cell layout against agg_ref."""
    d = _Dev(engine, h.ac)
    rows, cols = d.call(engine, h.ac)
    got = {"rows": rows.tolist(), "cols": [
        {n: [_signed(int(x)) if n in ("count", "first_ts", "last_ts")
             else int(x) for x in cols[0][n]] for n in ar.NAMES}]}
    assert not ar.check_against_hand(h, got)
    _check(h.ac, rows, cols)
    other = not h.ac.per_series
    rows, cols = d.call(engine, h.ac, per_series=other)
    _check(h.ac, rows, cols, per_series=other)
    d.free()


# ---------------------------------------------------- segment and tile edges

def _mixed_cols(r, n, null_rate=0.2):
    """One column of every type plus a predicate-only i64 column."""
    def valid():
        return r.random(n) >= null_rate
    return [
        fr.Col(fr.CT_F64, np.round(r.normal(50, 20, n), 2), valid()),
        fr.Col(fr.CT_I64, r.integers(-2**62, 2**62, n), valid()),
        fr.Col(fr.CT_U64, r.integers(0, 2**64, n, dtype=np.uint64), valid()),
        fr.Col(fr.CT_BOOL, r.integers(0, 2, n).astype(np.uint8), valid()),
        fr.Col(fr.CT_I64, r.integers(0, 10, n), None),   # predicate only
    ]


ALL4 = [(0, ar.NAMES), (1, ar.NAMES), (2, ar.NAMES), (3, ar.NAMES)]


@pytest.mark.parametrize("width", [100, 700])
def test_series_lengths_around_the_edges(engine, tile, width):
    """Series of 0, 1, 63 ... 3T+1 rows on a raw set, in an order that puts
    series ends at many places of the wave, the segment and the tile."""
    T = tile
    sizes = [65, 0, 1, 63, T - 1, 64, 511, T, 0, 0, 512, 513, T + 1, 1,
             3 * T + 1, 0]
    assert set(sizes) == {0, 1, 63, 64, 65, 511, 512, 513, T - 1, T, T + 1,
                          3 * T + 1}
    n = sum(sizes)
    assert n <= 20000
    r = np.random.default_rng(width)
    case = fr.Case(f"lengths w{width}", sizes, fr.group_ts(sizes, step=1),
                   _mixed_cols(r, n), [], [(4, "ge", 2)])
    nb = (3 * T + 1) // width + 2
    for ps in (True, False):
        _run(engine, ar.AggCase(case, ALL4, fr.T0 - 3, width, nb, ps))


def test_cell_boundaries_on_the_edges(engine, tile):
    """One series of 3T+1 rows with one row per nanosecond from t0: the
    bucket width is the row at which cells change.  64, 512 and T put the
    boundary exactly on a wave step, a segment and a tile, the widths next
    to them one row either side."""
    T = tile
    n = 3 * T + 1
    r = np.random.default_rng(3)
    case = fr.Case("boundaries", [n], fr.group_ts([n], step=1),
                   _mixed_cols(r, n), [], [(4, "ge", 1)])
    for w in (63, 64, 65, 511, 512, 513, T - 1, T, T + 1):
        ac = ar.AggCase(case._replace(name=f"boundary w{w}"), ALL4, fr.T0, w,
                        n // w + 1, True)
        _run(engine, ac)


def test_cell_across_segments_that_keep_nothing(engine, tile):
    """The middle series is one cell over nine segments; only rows of its
    first and last segment are kept, so the stitch crosses seven segments
    without a kept row.  Its neighbours share the segments at both ends."""
    seg = tile // 4
    sizes = [100, 9 * seg, 300]
    n = sum(sizes)
    r = np.random.default_rng(5)
    cols = _mixed_cols(r, n, 0.1)
    row = np.arange(n)
    mark = ((row < 100 + seg - 100) | (row >= 100 + 8 * seg)).astype(np.int64)
    cols[4] = fr.Col(fr.CT_I64, mark, None)
    case = fr.Case("empty middle", sizes, fr.group_ts(sizes, step=1), cols,
                   [], [(4, "eq", 1)])
    ref = _run(engine, ar.AggCase(case, ALL4, fr.T0, 10**6, 1, True))
    assert ref["rows"][1] == (seg - 100) + seg
    _run(engine, ar.AggCase(case, ALL4, fr.T0, 10**6, 1, False))


@pytest.mark.parametrize("k", [64, 65])
def test_one_row_series_in_one_wave_step(engine, k):
    sizes = [5] + [1] * k + [200]
    n = sum(sizes)
    r = np.random.default_rng(k)
    case = fr.Case(f"{k} one-row series", sizes, fr.group_ts(sizes, step=1),
                   _mixed_cols(r, n, 0.3), [], [(4, "ge", 3)])
    for ps in (True, False):
        _run(engine, ar.AggCase(case, ALL4, fr.T0, 50, 3, ps))


def test_empty_series_filtered_out_and_empty_set(engine):
    r = np.random.default_rng(9)
    sizes = [70, 0, 130]   # a series without rows between two others
    n = sum(sizes)
    case = fr.Case("empty series", sizes, fr.group_ts(sizes, step=1),
                   _mixed_cols(r, n), [], [(4, "ge", 5)])
    ref = _run(engine, ar.AggCase(case, ALL4, fr.T0, 40, 4, True))
    assert ref["rows"][4:8] == [0, 0, 0, 0] and sum(ref["rows"]) > 0
    # nothing kept: every cell holds the empty values
    none = case._replace(name="all filtered", preds=[(4, "gt", 100)])
    for ps in (True, False):
        ref = _run(engine, ar.AggCase(none, ALL4, fr.T0, 40, 4, ps))
        assert not any(ref["rows"])
    # a set without rows
    cols = [fr.Col(c.ctype, c.val[:0], None) for c in case.cols]
    zero = fr.Case("zero rows", [0, 0], np.zeros(0, np.int64), cols, [],
                   [(4, "ge", 5)])
    for ps in (True, False):
        ref = _run(engine, ar.AggCase(zero, ALL4, fr.T0, 40, 3, ps))
        assert ref["rows"] == [0] * (6 if ps else 3)


# ------------------------------------------------------- page sets, raw sets

def test_page_set_with_split_series_equals_raw_set(engine):
    """Series 0 and 2 are stored as several consecutive column groups: the
    cells are those of the raw set with one entry per series."""
    r = np.random.default_rng(21)
    groups_of = [(0, 700), (0, 64), (1, 513), (2, 1), (2, 900), (2, 300)]
    series = [764, 513, 1201]
    n = sum(series)
    ts = fr.group_ts(series, step=7)
    fv, iv, bv = r.random(n) >= 0.2, r.random(n) >= 0.4, r.random(n) >= 0.1
    f = np.round(r.normal(50, 10, n), 1)
    i = r.integers(-50, 50, n)
    b = r.integers(0, 2, n).astype(np.uint8)
    # the page decoders write null slots as zero: the case holds the same
    cols = [fr.Col(fr.CT_F64, np.where(fv, f, 0.0), fv,
                   [(int(ts[100]), int(ts[180]))]),
            fr.Col(fr.CT_I64, np.where(iv, i, 0), iv),
            fr.Col(fr.CT_BOOL, np.where(bv, b, 0).astype(np.uint8), bv)]
    case = fr.Case("pages", [m for _, m in groups_of], ts, cols, [],
                   [(1, "lt", 30)], (int(ts[3]), int(ts[-1])),
                   [(int(ts[400]), int(ts[420]))])
    aggs = [(0, ar.NAMES), (1, ar.NAMES), (2, ar.NAMES)]
    ac = ar.AggCase(case, aggs, fr.T0 + 50, 1500, 5, True, series)
    groups, lo = [], 0
    for sid, m in groups_of:
        sl = slice(lo, lo + m)
        groups.append((sid, [
            (gs.page_of(ts[sl], gs.CT_TIME), gs.CT_TIME),
            (gs.page_of(f[sl], gs.CT_F64, fv[sl]), gs.CT_F64),
            (gs.page_of(i[sl], gs.CT_I64, iv[sl]), gs.CT_I64),
            (gs.page_of(b[sl], gs.CT_BOOL, bv[sl]), gs.CT_BOOL)]))
        lo += m
    gset = engine.upload(groups)
    assert gset.ngroups == 6
    d = _Dev(engine, ac, gset=gset, nseries=3)
    d.ts = torch.zeros(n, dtype=torch.int64, device="cuda")
    engine.decode(gset, 0, d.ts)
    for k, dt in enumerate([torch.float64, torch.int64, torch.uint8]):
        val = torch.zeros(n, dtype=dt, device="cuda")
        vd = torch.zeros(n, dtype=torch.uint8, device="cuda")
        engine.decode(gset, 1 + k, val, vd)
        d.cols[k] = (d.cols[k][0], val, vd, d.cols[k][3])
    for ps in (True, False):
        p_rows, p_cols = d.call(engine, ac, per_series=ps)
        _check(ac, p_rows, p_cols, per_series=ps)
        raw = _Dev(engine, ac)
        r_rows, r_cols = raw.call(engine, ac, per_series=ps)
        raw.free()
        assert p_rows.tolist() == r_rows.tolist()
        for a, b2 in zip(p_cols, r_cols):
            for nm in ar.NAMES:
                assert a[nm].tolist() == b2[nm].tolist(), nm  # sums included
    gset.free()


# ------------------------------------------- columns and output patterns

@pytest.fixture(scope="module")
def pattern_case():
    """Nine columns (every type twice and a predicate-only one) over a few
    series, and its reference with every aggregate of the first eight."""
    r = np.random.default_rng(33)
    sizes = [300, 0, 129, 700, 64]
    n = sum(sizes)
    a, b = _mixed_cols(r, n), _mixed_cols(r, n, 0.5)
    cols = a[:4] + b[:4] + [a[4]]
    case = fr.Case("patterns", sizes, fr.group_ts(sizes, step=3), cols, [],
                   [(8, "ge", 3), (0, "is_not_null")], None,
                   [(fr.T0 + 300, fr.T0 + 420)])
    ac = ar.AggCase(case, [(c, ar.NAMES) for c in range(8)], fr.T0 + 10, 500,
                    4, True)
    return ac, {True: ar.agg_ref(ac),
                False: ar.agg_ref(ac._replace(per_series=False))}


def test_every_pattern_of_null_outputs(engine, pattern_case):
    """All 256 subsets of the eight output arrays, eight per call over the
    eight aggregated columns; d_rows NULL in every other call."""
    ac, refs = pattern_case
    d = _Dev(engine, ac)
    subsets = [tuple(n for k, n in enumerate(ar.NAMES) if m >> k & 1)
               for m in range(256)]
    seen = set()
    for call in range(32):
        aggs = [(c, subsets[call * 8 + c]) for c in range(8)]
        ps = call % 4 < 2
        rows, cols = d.call(engine, ac, aggs=aggs, per_series=ps,
                            want_rows=call % 2 == 0)
        assert (rows is None) == (call % 2 == 1)
        _check(ac, rows, cols, aggs, ps, ref=refs[ps])
        seen.update(names for _, names in aggs)
    d.free()
    assert len(seen) == 256


@pytest.mark.parametrize("naggs", [1, 2, 8])
def test_one_two_and_eight_columns(engine, pattern_case, naggs):
    """Column 8 only serves the predicate; the aggregated columns are taken
    from the back, so their order differs from cols[]; one column is
    aggregated twice when there are eight."""
    ac, refs = pattern_case
    picks = {1: [5], 2: [6, 1], 8: [7, 6, 5, 4, 3, 2, 1, 7]}[naggs]
    aggs = [(c, ar.NAMES) for c in picks]
    d = _Dev(engine, ac)
    for ps in (True, False):
        rows, cols = d.call(engine, ac, aggs=aggs, per_series=ps)
        ref = {"rows": refs[ps]["rows"],
               "cols": [refs[ps]["cols"][c] for c in picks]}
        _check(ac, rows, cols, aggs, ps, ref=ref)
    d.free()


# ------------------------------------------------------------- agreement

def test_agrees_with_filter_group_output(engine):
    """gs_filter_group's own device output, cut at its group offsets and
    reduced cell by cell, gives the same cells."""
    r = np.random.default_rng(41)
    sizes = [1500, 40, 2600, 0, 513]
    n = sum(sizes)
    cols = _mixed_cols(r, n)
    case = fr.Case("via filter", sizes, fr.group_ts(sizes, step=2), cols, [],
                   [(4, "ge", 4), (1, "is_not_null")],
                   (fr.T0 + 9, fr.T0 + 5000), [(fr.T0 + 700, fr.T0 + 800)])
    ac = ar.AggCase(case, ALL4, fr.T0 + 4, 600, 6, True)
    d = _Dev(engine, ac)
    rows, got = d.call(engine, ac)
    outs = [(torch.zeros(n * WIDTH[c.ctype], dtype=torch.uint8, device="cuda"),
             torch.zeros(n, dtype=torch.uint8, device="cuda"))
            for c in case.cols[:4]]
    o_ts = torch.zeros(n, dtype=torch.int64, device="cuda")
    fcols = [dc + (o[0], o[1]) for dc, o in zip(d.cols[:4], outs)] + [d.cols[4]]
    kept, offs = engine.filter_group(d.gset, d.ts, fcols, list(case.preds),
                                     (), case.time_range,
                                     list(case.row_tombs), d_out_ts=o_ts)
    d.free()
    assert 0 < kept < n
    f_ts = o_ts.cpu().numpy()[:kept]
    ncell = len(sizes) * ac.n_buckets
    for k, (c, (o_val, o_valid)) in enumerate(zip(case.cols[:4], outs)):
        val = o_val.cpu().numpy().view(fr.NP_DTYPE[c.ctype])[:kept]
        valid = o_valid.cpu().numpy()[:kept]
        cells = [[] for _ in range(ncell)]
        n_rows = [0] * ncell
        for s in range(len(sizes)):
            for j in range(offs[s], offs[s + 1]):
                b = ar.bucket_of(f_ts[j], ac.t0, ac.bucket_ns, ac.n_buckets)
                if b is None:
                    continue
                n_rows[s * ac.n_buckets + b] += 1
                if valid[j]:
                    cells[s * ac.n_buckets + b].append(
                        (int(f_ts[j]), fr.bits(c.ctype, val[j])))
        assert rows.tolist() == n_rows
        for i, cell in enumerate(cells):
            want = ar.reduce_rows(c.ctype, cell)
            for nm in ar.NAMES:
                g = int(got[k][nm][i])
                if nm == "sum":
                    assert ar.sum_within(c.ctype, g, want["sum"],
                                         want["count"], want["sum_abs"])
                else:
                    assert g == want[nm] & ar.M64, (k, i, nm)


def test_agrees_with_gs_scan(engine):
    """One f64 column, one value predicate, tombstones and a time range,
    reduced over the series: count and max equal gs_scan's aggregate, sum
    within rtol 1e-12 (positive data)."""
    r = np.random.default_rng(17)
    sizes = [4096, 1000, 2500]
    n = sum(sizes)
    ts = fr.group_ts(sizes)
    val = np.round(np.clip(r.normal(50, 25, n), 0.1, 100), 1)
    tombs = [(int(ts[100]), int(ts[400])), (int(ts[900]), int(ts[900]))]
    rng = (int(ts[50]), int(ts[3000]))
    nb, bn = 7, 500 * 10**9
    groups, lo = [], 0
    for g, m in enumerate(sizes):
        sl = slice(lo, lo + m)
        groups.append((g, [(gs.page_of(ts[sl], gs.CT_TIME), gs.CT_TIME),
                           (gs.page_of(val[sl], gs.CT_F64), gs.CT_F64)]))
        lo += m
    gset = engine.upload(groups)
    s_ts = torch.zeros(n, dtype=torch.int64, device="cuda")
    s_val = torch.zeros(n, dtype=torch.float64, device="cuda")
    agg = dict(bucket_ns=bn, t0=fr.T0, n_buckets=nb,
               d_max=torch.full((nb,), -np.inf, dtype=torch.float64,
                                device="cuda"),
               d_sum=torch.zeros(nb, dtype=torch.float64, device="cuda"),
               d_count=torch.zeros(nb, dtype=torch.int64, device="cuda"))
    engine.scan(gset, s_ts, s_val, time_range=rng, tombstones=tombs, agg=agg,
                value_pred=("gt", 40.0))
    d_ts = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_val = torch.zeros(n, dtype=torch.float64, device="cuda")
    engine.decode(gset, 0, d_ts)
    engine.decode(gset, 1, d_val)
    out = {k: _poison(nb * 8) for k in ("count", "sum", "max")}
    engine.agg_group(gset, d_ts, [(gs.CT_F64, d_val)], [(0, "gt", 40.0)],
                     [(0, out)], fr.T0, bn, nb, per_series=False,
                     time_range=rng, row_tombstones=tombs)
    gset.free()
    count = out["count"].cpu().numpy().view(np.int64)
    assert count.tolist() == agg["d_count"].cpu().numpy().tolist()
    assert 0 < count.sum() < n and (count > 0).sum() >= 3
    assert (out["max"].cpu().numpy().view(np.uint64).tolist() ==
            agg["d_max"].cpu().numpy().view(np.uint64).tolist())
    np.testing.assert_allclose(out["sum"].cpu().numpy().view(np.float64),
                               agg["d_sum"].cpu().numpy(), rtol=1e-12, atol=0)


def test_same_bits_twice_and_under_any_grid(engine, tile):
    """Two identical calls, and calls capped at 1 and at 3 blocks, give the
    uncapped call's bits in every array, the f64 sum included."""
    r = np.random.default_rng(52)
    sizes = [3 * tile + 5, 700, 2 * tile, 64, 1, 4000]
    n = sum(sizes)
    assert n <= 20000
    case = fr.Case("grids", sizes, fr.group_ts(sizes, step=1),
                   _mixed_cols(r, n), [], [(4, "ge", 2)])
    for ps in (True, False):
        ac = ar.AggCase(case, ALL4, fr.T0, 900, 5, ps)
        d = _Dev(engine, ac)
        base_rows, base = d.call(engine, ac)
        _check(ac, base_rows, base)
        runs = [d.call(engine, ac)]
        for cap in (1, 3):
            with gs.grid_cap(cap):
                runs.append(d.call(engine, ac))
                assert gs.grid_rounds() > 1  # the cap was felt
        d.free()
        for rows, cols in runs:
            assert rows.tolist() == base_rows.tolist()
            for a, b in zip(cols, base):
                for nm in ar.NAMES:
                    assert a[nm].tolist() == b[nm].tolist(), (ps, nm)


# --------------------------------------------------------------------- fuzz

@pytest.mark.parametrize("chunk", range(5))
def test_fuzz(engine, chunk):
    for seed in list(ar.FUZZ_SEEDS)[chunk * 10:(chunk + 1) * 10]:
        ac = ar.fuzz_case(seed)
        _run(engine, ac, want_rows=seed % 3 != 0)


# ------------------------------------------------------------------- errors

def _good():
    r = np.random.default_rng(1)
    sizes = [40, 60]
    case = fr.Case("good", sizes, fr.group_ts(sizes),
                   [fr.Col(fr.CT_I64, r.integers(0, 9, 100), None)],
                   [fr.StrCol([b"x%d" % i for i in range(100)], None)],
                   [(0, "ge", 4)])
    return ar.AggCase(case, [(0, ar.NAMES)], fr.T0, 10**10, 3, True)


def test_errors_leave_outputs_and_engine_alone(engine):
    ac = _good()
    d = _Dev(engine, ac)
    ncell = 2 * 3
    out = {n: _poison(ncell * 8) for n in ar.NAMES}
    d_rows = _poison(ncell * 8)
    col = d.cols[0]
    ok = dict(gset=d.gset, d_ts=d.ts, cols=[col], preds=[(0, "ge", 4)],
              aggs=[(0, out)], t0=fr.T0, bucket_ns=10**10, n_buckets=3,
              per_series=True, str_cols=d.strs)
    big = engine.raw_set(np.array([1] * 70000, np.int64))
    bad_calls = {
        # what gs_filter_group refuses
        "no columns": dict(ok, cols=[], str_cols=[], preds=[]),
        "33 columns": dict(ok, cols=[col] * 32),
        "17 predicates": dict(ok, preds=[(0, "ge", 4)] * 17),
        "time ctype": dict(ok, cols=[(0,) + col[1:]]),
        "string ctype in a fixed column": dict(ok, cols=[(5,) + col[1:]]),
        "unknown ctype": dict(ok, cols=[(9,) + col[1:]]),
        "predicate column too large": dict(ok, preds=[(2, "is_null")]),
        "predicate column negative": dict(ok, preds=[(-1, "is_null")]),
        "comparison on a string column": dict(ok, preds=[(1, "eq")]),
        "op 0": dict(ok, preds=[(0, 0, 4)]),
        "op 10": dict(ok, preds=[(0, 10, 4)]),
        "NULL d_ts": dict(ok, d_ts=None),
        "NULL d_val": dict(ok, cols=[(col[0], None) + col[2:]]),
        # its own
        "no aggregates": dict(ok, aggs=[]),
        "33 aggregates": dict(ok, aggs=[(0, out)] * 33),
        "aggregated column negative": dict(ok, aggs=[(-1, out)]),
        "aggregated column is the string column": dict(ok, aggs=[(1, out)]),
        "aggregated column too large": dict(ok, aggs=[(2, out)]),
        "n_buckets 0": dict(ok, n_buckets=0),
        "n_buckets negative": dict(ok, n_buckets=-3),
        "bucket_ns negative": dict(ok, bucket_ns=-1),
        "bucket_ns 0 with two buckets": dict(ok, bucket_ns=0, n_buckets=2),
        "too many cells": dict(ok, gset=big, n_buckets=2**15),
    }
    for name, kw in bad_calls.items():
        with pytest.raises(RuntimeError) as ei:
            engine.agg_group(kw["gset"], kw["d_ts"], kw["cols"], kw["preds"],
                             kw["aggs"], kw["t0"], kw["bucket_ns"],
                             kw["n_buckets"], kw["per_series"],
                             kw["str_cols"], d_rows=d_rows)
        assert ei.value.status == GS_ERR, name
        assert "gs_agg_group" in str(ei.value), name
        for t in list(out.values()) + [d_rows]:
            assert (t.cpu().numpy() == POISON).all(), name
        _run(engine, ac)  # the engine is usable: a good call right after
    assert len(bad_calls) == 23
    big.free()
    d.free()


def test_unsorted_series_is_a_format_error(engine):
    """One timestamp out of order inside a series: GS_ERR_FORMAT, an error
    return; equal timestamps are refused as well; the same timestamps
    across a series boundary are fine."""
    ac = _good()
    for at, delta in ((17, -2 * 10**9), (70, -10**9)):
        ts = np.array(ac.case.ts)
        ts[at] += delta
        bad = ac._replace(case=ac.case._replace(ts=ts))
        d = _Dev(engine, bad)
        with pytest.raises(RuntimeError) as ei:
            d.call(engine, bad)
        d.free()
        assert ei.value.status == GS_ERR_FORMAT, at
        assert "gs_agg_group" in str(ei.value)
        _run(engine, ac)
    # series 1 starts below the end of series 0: no violation
    assert ac.case.ts[40] < ac.case.ts[39]
