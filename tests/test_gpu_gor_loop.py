"""Row loop of the fused Gorilla decode (k_gor_chunks_filtered, with and
without the bucket aggregate), through Engine.scan and scan_fields_async,
against the oracle's decode of the same pages plus a numpy span/bucket
composition.

Rows are bit-exact as uint64, count and max exact, sum within rtol=1e-12,
and two identical runs are bit-identical.

The shapes are the smallest that reach every way the loop can end a lane:
pages of 2 to 4500 rows mixed in one set, so one wave holds chunks of 1, 2,
15, 16, 17, 404, 2047 and 2048 rows that finish at different iterations
(parked lanes, a last partial ring, single-row chunks); spans that start
mid-ring, end on a chunk's first row, one row before a chunk's last row,
inside a chunk that may stop early and inside a page's last chunk; value
streams of 1 bit per value, of 64 meaningful bits, and of full-precision
doubles; bucket grids on and off the 16-iteration flush cadence.

A time page of one row is not RLE-encoded (the format has no delta to
repeat), and one such page takes the whole set off the fused scan.  Pages
of a single row therefore have a test of their own on the general path;
the sets of the other tests prove at upload that they are fused-capable.

Expected bucket sums are exactly rounded (math.fsum), so the tolerance is
spent on the engine's rounding alone, also where the terms cancel."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = 1_700_000_000 * NS

# page row counts of one series; series s uses the list rotated by 2*s, so
# the same row span meets different chunk positions in every series
PAGE_ROWS = [4097, 2, 2048, 15, 4500, 2049, 16, 2047, 17]
NSERIES = 4
N_ALL = sum(PAGE_ROWS)  # 14811 rows per series


def _walk(rng, n):
    return np.round(np.clip(np.cumsum(rng.normal(0, 0.5, n)) + 50, 0, 100), 1)


def _constant(rng, n):
    return np.full(n, 42.5)


def _uniform(rng, n):
    # full-precision doubles, all of one sign: a relative bound on a sum
    # means nothing once terms cancel
    return rng.uniform(0.0, 1e3, n)


def _alternating(rng, n):
    v = np.empty(n, dtype=np.uint64)
    v[0::2] = 0x3FF0000000000001
    v[1::2] = 0xBFF0000000000000
    return v.view(np.float64)


def _nans(rng, n):
    v = _walk(rng, n)
    nan = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
    v[5::97] = nan
    v[n // 3:n // 3 + 40] = 100.0
    v[n // 3 + 10] = nan
    return v


VALUES = {"walk": _walk, "constant": _constant, "uniform": _uniform,
          "alternating": _alternating, "nans": _nans}

# closed row ranges of a series, None = nothing selected.  Series 0 has its
# 4097-row page at rows 0..4096 (chunks 0..2047, 2048..4095, 4096) and its
# 4500-row page at rows 6162..10661 (last chunk from 10258).
SPANS = [
    (0, N_ALL - 1),     # everything
    None,               # empty
    (7000, 7000),       # a single row
    (2053, N_ALL - 1),  # starts at row 5 of a chunk: mid-ring
    (0, 2048),          # ends exactly on a chunk's first row
    (100, 2046),        # ends one row before a chunk's last row
    (3, 1000),          # ends inside a chunk that may stop early
    (6000, 10357),      # ends inside a page's last chunk
]

# (bucket seconds, t0 offset in seconds, n_buckets); rows are 1 s apart
BUCKETS = [
    (16, 0, N_ALL // 16 + 1),   # a boundary on every 16th iteration
    (16, -1, N_ALL // 16 + 2),  # the same, one row off the cadence
    (5, -3, N_ALL // 5 + 2),    # several boundaries per ring
    (1_000_000, -17, 1),        # one bucket longer than the series
]


def _page_data(pg, n, dec):
    pg = np.frombuffer(pg, np.uint8)
    hdr = int.from_bytes(pg[0:4].tobytes(), "big")
    return dec(pg[16 + hdr:].tobytes(), n)


def _build(maker, seed, nf, page_rows=PAGE_ROWS, nseries=NSERIES):
    """Groups of one set + the oracle's decode of those very pages."""
    import cnosdb_amd as gs
    from oracle import pyoracle as orc

    rng = np.random.default_rng(seed)
    groups, truth = [], []
    for s in range(nseries):
        k = (2 * s) % len(page_rows)
        rows = page_rows[k:] + page_rows[:k]
        n_all = sum(rows)
        ts = T0 + np.arange(n_all, dtype=np.int64) * NS
        vals = [maker(rng, n_all) for _ in range(nf)]
        dts, dvals, r0 = [], [[] for _ in range(nf)], 0
        for n in rows:
            tp = gs.page_of(ts[r0:r0 + n], gs.CT_TIME)
            pages = [(tp, gs.CT_TIME)]
            dts.append(_page_data(tp, n, orc.decode_i64))
            for f in range(nf):
                vp = gs.page_of(vals[f][r0:r0 + n], gs.CT_F64)
                pages.append((vp, gs.CT_F64))
                dvals[f].append(_page_data(vp, n, orc.decode_f64))
            groups.append((s, pages))
            r0 += n
        truth.append((np.concatenate(dts),
                      [np.concatenate(v) for v in dvals]))
    return groups, truth


def _range_of(span):
    if span is None:
        return T0 - 500 * NS, T0 - 100 * NS
    # closed range that starts and ends between two rows
    return T0 + span[0] * NS - NS // 2, T0 + span[1] * NS + NS // 3


def _bucket_sums(b, v, nb):
    """Exactly rounded sum of v per bucket index b."""
    out = np.zeros(nb)
    order = np.argsort(b, kind="stable")
    bs, vs = b[order], v[order]
    cut = np.flatnonzero(np.diff(bs)) + 1
    for s, e in zip(np.concatenate(([0], cut)),
                    np.concatenate((cut, [bs.size]))):
        if e > s:
            out[bs[s]] = math.fsum(vs[s:e])
    return out


def _expect(truth, nf, lo, hi, bucket=None):
    """numpy composition: closed-range filter, compaction, bucket agg with
    the engine's max rule (x > mx: a NaN never wins, the sum carries it)."""
    out_ts, out_val = [], [[] for _ in range(nf)]
    if bucket:
        bucket_s, t0_off, nb = bucket
        t0, bucket_ns = T0 + t0_off * NS, bucket_s * NS
        mx = np.full((nf, nb), -np.inf)
        ct = np.zeros((nf, nb), dtype=np.int64)
        sel_b, sel_v = [], [[] for _ in range(nf)]
    for ts, vals in truth:
        s = np.searchsorted(ts, lo, side="left")
        e = np.searchsorted(ts, hi, side="right")
        t = ts[s:e]
        out_ts.append(t)
        for f in range(nf):
            out_val[f].append(vals[f][s:e])
        if not bucket:
            continue
        b = (t - t0) // bucket_ns
        m = (b >= 0) & (b < nb)
        for f in range(nf):
            v = vals[f][s:e]
            np.add.at(ct[f], b[m], 1)
            sel_v[f].append(v[m])
            ok = m & ~np.isnan(v)
            np.maximum.at(mx[f], b[ok], v[ok])
        sel_b.append(b[m])
    exp = dict(ts=np.concatenate(out_ts),
               val=np.stack([np.concatenate(v) for v in out_val]))
    if bucket:
        sel_b = np.concatenate(sel_b)
        sm = np.stack([_bucket_sums(sel_b, np.concatenate(sel_v[f]), nb)
                       for f in range(nf)])
        exp.update(mx=mx, sm=sm, ct=ct)
    return exp


class _Scanner:
    """One uploaded set with its device buffers, scanned many times."""

    def __init__(self, eng, groups, nf, fused=True):
        import torch
        self.eng, self.nf = eng, nf
        self.gset = eng.upload(groups)
        rows = self.rows = self.gset.rows
        self.d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
        self.d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
        self.d_ots = torch.zeros(rows, dtype=torch.int64, device="cuda")
        self.d_oval = torch.zeros(nf * rows, dtype=torch.float64,
                                  device="cuda")
        if fused:
            # gs_scan_fields refuses a set that would leave the fused scan
            self.scan(*_range_of(None), None, True)

    def free(self):
        self.gset.free()

    def scan(self, lo, hi, bucket, use_async):
        import torch
        import cnosdb_amd as gs
        nf, rows, agg = self.nf, self.rows, None
        if bucket:
            bucket_s, t0_off, nb = bucket
            agg = dict(bucket_ns=bucket_s * NS, t0=T0 + t0_off * NS,
                       n_buckets=nb,
                       d_max=torch.full((nf * nb,), -np.inf,
                                        dtype=torch.float64, device="cuda"),
                       d_sum=torch.zeros(nf * nb, dtype=torch.float64,
                                         device="cuda"),
                       d_count=torch.zeros(nf * nb, dtype=torch.int64,
                                           device="cuda"))
        self.d_ots.zero_()
        self.d_oval.zero_()
        if use_async:
            gs.scan_fields_async(self.eng, self.gset, list(range(nf)),
                                 self.d_ts, self.d_val, (lo, hi), self.d_ots,
                                 self.d_oval, agg=agg)
            res = self.eng.scan_wait(self.gset)
        else:
            assert nf == 1
            res = self.eng.scan(self.gset, self.d_ts, self.d_val,
                                time_range=(lo, hi), d_out_ts=self.d_ots,
                                d_out_val=self.d_oval, agg=agg)
        n = int(res.out_rows)
        got = dict(
            ts=self.d_ots[:n].cpu().numpy(),
            val=np.stack([self.d_oval[f * rows:f * rows + n].cpu().numpy()
                          for f in range(nf)]))
        if bucket:
            got.update(mx=agg["d_max"].cpu().numpy().reshape(nf, nb),
                       sm=agg["d_sum"].cpu().numpy().reshape(nf, nb),
                       ct=agg["d_count"].cpu().numpy().reshape(nf, nb))
        return got


def _same_sum(got, exp, what):
    nan = np.isnan(exp)
    assert (np.isnan(got) == nan).all(), what
    err = np.abs(got[~nan] - exp[~nan])
    assert (err <= 1e-12 * np.abs(exp[~nan])).all(), what


def _check(got, exp, what):
    assert got["ts"].size == exp["ts"].size, what
    assert (got["ts"] == exp["ts"]).all(), what
    assert (got["val"].view(np.uint64)
            == exp["val"].view(np.uint64)).all(), what
    if "ct" in exp:
        assert (got["ct"] == exp["ct"]).all(), what
        assert (got["mx"].view(np.uint64)
                == exp["mx"].view(np.uint64)).all(), what
        _same_sum(got["sm"], exp["sm"], what)


def _run_all(sc, truth, nf, use_async, buckets, name, spans=SPANS):
    for si, span in enumerate(spans):
        lo, hi = _range_of(span)
        for bucket in [None] + buckets:
            what = f"{name} span {si} bucket {bucket}"
            a = sc.scan(lo, hi, bucket, use_async)
            b = sc.scan(lo, hi, bucket, use_async)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (what, k)
            _check(a, _expect(truth, nf, lo, hi, bucket), what)


@pytest.fixture(scope="module")
def engine():
    import cnosdb_amd as gs
    e = gs.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", list(VALUES))
def test_scan_matches_oracle(engine, name):
    """Engine.scan, one field: every span, without and with each grid."""
    groups, truth = _build(VALUES[name], sum(map(ord, name)), 1)
    sc = _Scanner(engine, groups, 1)
    try:
        _run_all(sc, truth, 1, False, BUCKETS, name)
    finally:
        sc.free()


@pytest.mark.parametrize("name", list(VALUES))
def test_scan_fields_async_matches_oracle(engine, name):
    """scan_fields_async over two fields: every span, without aggregate
    and with the two grids that put most boundaries into a ring."""
    groups, truth = _build(VALUES[name], 7 + sum(map(ord, name)), 2)
    sc = _Scanner(engine, groups, 2)
    try:
        _run_all(sc, truth, 2, True, [BUCKETS[0], BUCKETS[2]], name)
    finally:
        sc.free()


def test_truncated_page_among_valid_pages(engine):
    """One page cut at 60 % of its stream (inside its second chunk) among
    valid pages: a span that covers the cut raises; a span that ends before
    it, in chunks that may stop early, returns every page's rows exactly —
    with and without the aggregate."""
    import cnosdb_amd as gs

    page_rows = [4500, 2049]
    groups, truth = _build(_walk, 99, 1, page_rows=page_rows, nseries=3)
    # the rotation leaves series 1's 4500-row page first
    gi = len(page_rows)  # group index of series 1, page 0
    sid, pages = groups[gi]
    vals = truth[1][1][0][:4500]
    data = gs.encode_f64(vals)
    cut = data[:int(len(data) * 0.6)]
    groups[gi] = (sid, [pages[0], (gs.build_page(cut, 4500), gs.CT_F64)])
    sc = _Scanner(engine, groups, 1)
    try:
        for bucket in (None, BUCKETS[2]):
            lo, hi = _range_of((3, 1000))
            for use_async in (False, True):
                got = sc.scan(lo, hi, bucket, use_async)
                _check(got, _expect(truth, 1, lo, hi, bucket),
                       f"before the cut, bucket {bucket}")
            lo, hi = _range_of((0, sum(page_rows) - 1))
            with pytest.raises(RuntimeError):
                sc.scan(lo, hi, bucket, False)
            with pytest.raises(RuntimeError):
                sc.scan(lo, hi, bucket, True)
            # the error does not stick: the narrow span still decodes
            lo, hi = _range_of((3, 1000))
            got = sc.scan(lo, hi, bucket, False)
            _check(got, _expect(truth, 1, lo, hi, bucket), "after the error")
    finally:
        sc.free()


def test_single_row_pages(engine):
    """Pages of one row among longer ones.  Their time pages are not RLE,
    so this set is scanned on the general path: same bar, other kernels."""
    page_rows = [1, 17, 1, 2048, 1]
    groups, truth = _build(_walk, 5, 1, page_rows=page_rows, nseries=3)
    sc = _Scanner(engine, groups, 1, fused=False)
    n = sum(page_rows)
    try:
        _run_all(sc, truth, 1, False, [(5, -3, n // 5 + 2)], "single rows",
                 spans=[(0, n - 1), None, (0, 0), (18, 18), (10, 1000)])
    finally:
        sc.free()
