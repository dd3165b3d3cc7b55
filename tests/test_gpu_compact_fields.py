"""gs_compact_merge_fields: compaction merge over every field column of a
column group (BatchMergeBuilder::take_last_and_merge,
reader/batch_builder.rs:132-155 — per column the newest non-null value
wins) vs the oracle restatement.  gs_compact_merge is the same kernel at
ncols=1, so the per-column comparisons below show that a column's result
does not depend on its neighbours; the oracle is what says it is right.

The oracle merges one float64 column; it serves every column type by
merging global source-row ids (exact in float64 at these sizes) and
gathering the expected bits of whatever dtype from the winning row."""
import numpy as np
import pytest
import torch

import cnosdb_amd as gs
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000_000
NS = 1_000_000_000
GRID = T0 + np.arange(20000, dtype=np.int64) * NS
STRIDE = 1 << 20  # source-row id = stream * STRIDE + row within (stream, series)
DTYPES = ("f64", "i64", "u64", "bool")


@pytest.fixture(scope="module")
def engine():
    e = gs.Engine(0)
    yield e
    e.close()


# ---------------------------------------------------------------- data

def _gen_vals(r, dtype, n):
    """Values as stored bits: uint64 for the 8-byte types, uint8 for bool."""
    if dtype == "f64":
        return np.round(r.normal(50, 10, n), 1).view(np.uint64)
    if dtype == "i64":
        v = r.integers(-1000, 1000, n, dtype=np.int64)
        return (v + np.where(r.random(n) < 0.5, 1 << 62, -(1 << 62))).view(
            np.uint64)
    if dtype == "u64":
        return (np.uint64(1 << 63) +
                r.integers(0, 1 << 40, n, dtype=np.int64).astype(np.uint64))
    return r.integers(0, 2, n, dtype=np.uint8)


def _mk_streams(r, sizes, nseries, dtypes, null_rates, absent=()):
    """streams[f][s] = (ts, [(bits, valid_or_None) or None per column]);
    sizes[f] = rows per series of stream f; absent = {(f, c)}."""
    streams = []
    for f, n in enumerate(sizes):
        per = []
        for s in range(nseries):
            ts = GRID[np.sort(r.choice(GRID.size, size=n, replace=False))]
            cols = []
            for c, dt in enumerate(dtypes):
                if (f, c) in absent:
                    cols.append(None)
                    continue
                valid = (r.random(n) >= null_rates[c]) if null_rates[c] else None
                cols.append((_gen_vals(r, dt, n), valid))
            per.append((ts, cols))
        streams.append(per)
    return streams


def _torch_dtype(dt):
    return {"f64": torch.float64, "i64": torch.int64, "u64": torch.int64,
            "bool": torch.uint8}[dt]


def _dev(bits, dt):
    if dt == "bool":
        return torch.from_numpy(np.ascontiguousarray(bits)).cuda()
    view = np.float64 if dt == "f64" else np.int64
    return torch.from_numpy(np.ascontiguousarray(bits).view(view)).cuda()


def _upload_raw(engine, per_series, dtypes):
    """One stream as a raw set over device arrays built on the host."""
    counts = np.array([t.size for t, _ in per_series], dtype=np.int64)
    gset = engine.raw_set(counts)
    d_ts = torch.from_numpy(np.concatenate([t for t, _ in per_series])).cuda()
    cols = []
    for c, dt in enumerate(dtypes):
        if per_series[0][1][c] is None:
            cols.append((None, None))
            continue
        bits = np.concatenate([cs[c][0] for _, cs in per_series])
        d_v = _dev(bits, dt)
        d_vd = None
        if any(cs[c][1] is not None for _, cs in per_series):
            vd = np.concatenate([
                (cs[c][1] if cs[c][1] is not None
                 else np.ones(t.size, bool)) for t, cs in per_series])
            d_vd = torch.from_numpy(vd.astype(np.uint8)).cuda()
        cols.append((d_v, d_vd))
    return gset, d_ts, cols


def _upload_tsm(engine, per_series, dtypes):
    """One stream as TSM pages (f64 columns only), decoded by gs_decode."""
    assert all(dt == "f64" for dt in dtypes)
    groups = []
    for s, (ts, cs) in enumerate(per_series):
        pages = [(gs.page_of(ts, gs.CT_TIME), gs.CT_TIME)]
        for bits, valid in cs:
            pages.append((gs.page_of(bits.view(np.float64), gs.CT_F64, valid),
                          gs.CT_F64))
        groups.append((s, pages))
    gset = engine.upload(groups)
    d_ts = torch.zeros(gset.rows, dtype=torch.int64, device="cuda")
    engine.decode(gset, 0, d_ts)
    cols = []
    for c in range(len(dtypes)):
        d_v = torch.zeros(gset.rows, dtype=torch.float64, device="cuda")
        d_vd = torch.zeros(gset.rows, dtype=torch.uint8, device="cuda")
        engine.decode(gset, 1 + c, d_v, d_vd)
        cols.append((d_v, d_vd))
    return gset, d_ts, cols


class _Merged:
    pass


def _merge(engine, streams, dtypes, tsm=(), out_valid=True, drop_valid=False):
    """Upload (stream f through TSM pages if f in tsm, else as a raw set),
    run compact_merge_fields, return host copies."""
    k = len(streams)
    gsets, tss, cols = [], [], []
    for f in range(k):
        up = _upload_tsm if f in tsm else _upload_raw
        g, t, cs = up(engine, streams[f], dtypes)
        if drop_valid:
            cs = [(v, None) for v, _ in cs]
        gsets.append(g)
        tss.append(t)
        cols.append(cs)
    total = sum(g.rows for g in gsets)
    d_ots = torch.zeros(total, dtype=torch.int64, device="cuda")
    outs = []
    for dt in dtypes:
        # poison so that a cell the kernel never stores cannot pass
        d_v = torch.full((total,), 0x5A, dtype=torch.uint8, device="cuda") \
            if dt == "bool" else \
            torch.full((total,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64,
                       device="cuda").view(_torch_dtype(dt))
        d_vd = torch.full((total,), 0x5A, dtype=torch.uint8, device="cuda") \
            if out_valid else None
        outs.append((d_v, d_vd))
    m = _Merged()
    m.out_rows, m.offs = engine.compact_merge_fields(gsets, tss, cols, d_ots,
                                                     outs)
    m.ts = d_ots[:m.out_rows].cpu().numpy()
    m.bits, m.valid = [], []
    for dt, (d_v, d_vd) in zip(dtypes, outs):
        h = d_v[:m.out_rows].cpu().numpy()
        m.bits.append(h if dt == "bool" else h.view(np.uint64))
        m.valid.append(d_vd[:m.out_rows].cpu().numpy()
                       if d_vd is not None else None)
    m.gsets, m.tss, m.cols, m.total = gsets, tss, cols, total
    return m


def _free(m):
    for g in m.gsets:
        g.free()


# -------------------------------------------------------------- oracle

def _expect(streams, s, c, all_valid=False):
    """Oracle merge of column c of series s through source-row ids:
    (uts, winning stream, winning row, valid)."""
    per = []
    for f in range(len(streams)):
        ts, cs = streams[f][s]
        ids = (f * STRIDE + np.arange(ts.size)).astype(np.float64)
        if cs[c] is None:  # absent column = all-null stream
            valid = np.zeros(ts.size, bool)
        else:
            valid = None if all_valid else cs[c][1]
        per.append((ts, ids, valid))
    uts, ids, valid = orc.merge_dedup(per)
    ids = ids.astype(np.int64)
    return uts, ids // STRIDE, ids % STRIDE, valid


def _expected_bits(streams, s, c, dtype, src_f, src_j, valid):
    exp = np.zeros(valid.size, dtype=np.uint8 if dtype == "bool" else np.uint64)
    for f in range(len(streams)):
        cs = streams[f][s][1]
        if cs[c] is None:
            continue
        m = valid & (src_f == f)
        exp[m] = cs[c][0][src_j[m]]
    return exp


def _newest_holder(streams, s):
    """Per merged timestamp, the newest stream that contains it."""
    per = [(streams[f][s][0], np.full(streams[f][s][0].size, float(f)), None)
           for f in range(len(streams))]
    _, newest, _ = orc.merge_dedup(per)
    return newest.astype(np.int64)


def _check(m, streams, dtypes, nseries, all_valid=False, tag=""):
    exp_rows = 0
    for s in range(nseries):
        lo, hi = m.offs[s], m.offs[s + 1]
        for c, dt in enumerate(dtypes):
            uts, sf, sj, valid = _expect(streams, s, c, all_valid)
            if c == 0:
                exp_rows += uts.size
                assert hi - lo == uts.size, f"{tag} series {s} rows"
                assert (m.ts[lo:hi] == uts).all(), f"{tag} series {s} ts"
            exp = _expected_bits(streams, s, c, dt, sf, sj, valid)
            got = m.bits[c][lo:hi]
            if m.valid[c] is not None:
                assert (m.valid[c][lo:hi] == valid.astype(np.uint8)).all(), \
                    f"{tag} series {s} col {c} validity"
            # null cells are expected as zero bits
            assert got.tolist() == exp.tolist(), f"{tag} series {s} col {c}"
    assert m.out_rows == exp_rows == m.offs[nseries]


def _per_column_merge(engine, m, c):
    """Column c merged alone through gs_compact_merge: the group kernel at
    ncols=1.  Equality with the group result shows independence from the
    other columns, not correctness; every caller also runs _check."""
    d_ots = torch.zeros(m.total, dtype=torch.int64, device="cuda")
    d_oval = torch.zeros(m.total, dtype=torch.float64, device="cuda")
    d_ovd = torch.zeros(m.total, dtype=torch.uint8, device="cuda")
    rows, offs = engine.compact_merge(
        m.gsets, m.tss, [cs[c][0] for cs in m.cols],
        [cs[c][1] for cs in m.cols], d_ots, d_oval, d_ovd)
    return (rows, offs, d_ots[:rows].cpu().numpy(),
            d_oval[:rows].cpu().numpy().view(np.uint64),
            d_ovd[:rows].cpu().numpy())


# --------------------------------------------------------------- tests

def test_truth_table(engine):
    """3 streams (0 oldest), 5 timestamps, 2 columns; N = null."""
    N = None
    t = [T0 + i * NS for i in range(5)]
    #          ts        col0  col1
    s0 = [(t[0], 1.5, 10), (t[1], 2.5, 20), (t[2], N, N), (t[3], 4.5, N)]
    s1 = [(t[0], 11.5, N), (t[2], N, N), (t[3], N, 31)]
    s2 = [(t[0], N, 42), (t[1], 22.5, N), (t[4], 55.5, N)]
    expected = [
        # t0: col0 newer null (s2) falls through to s1, which beats the
        #     older valid s0; col1 resolves to s2 — a different stream
        (t[0], (11.5, 1), (42, 1)),
        # t1: newer valid (s2) beats older valid (s0); col1 falls to s0
        (t[1], (22.5, 1), (20, 1)),
        # t2: null in every stream -> value 0, validity 0
        (t[2], (0.0, 0), (0, 0)),
        # t3: col0 from s0 below a newer null; col1 from s1
        (t[3], (4.5, 1), (31, 1)),
        # t4: timestamp present in only one stream; its col1 is null
        (t[4], (55.5, 1), (0, 0)),
    ]
    streams = []
    for rows in (s0, s1, s2):
        ts = np.array([r[0] for r in rows], dtype=np.int64)
        v0 = np.array([r[1] if r[1] is not None else -1.0 for r in rows])
        v1 = np.array([r[2] if r[2] is not None else -1 for r in rows],
                      dtype=np.int64)
        streams.append([(ts, [
            (v0.view(np.uint64), np.array([r[1] is not None for r in rows])),
            (v1.view(np.uint64), np.array([r[2] is not None for r in rows])),
        ])])
    m = _merge(engine, streams, ("f64", "i64"))
    assert m.out_rows == 5 and m.offs.tolist() == [0, 5]
    assert m.ts.tolist() == [e[0] for e in expected]
    assert m.bits[0].view(np.float64).tolist() == [e[1][0] for e in expected]
    assert m.valid[0].tolist() == [e[1][1] for e in expected]
    assert m.bits[1].view(np.int64).tolist() == [e[2][0] for e in expected]
    assert m.valid[1].tolist() == [e[2][1] for e in expected]
    _free(m)


def test_single_f64_column_equals_compact_merge(engine):
    r = np.random.default_rng(101)
    nseries, k = 3, 8
    sizes = [2000 + 50 * f for f in range(k)]
    streams = _mk_streams(r, sizes, nseries, ("f64",), (0.3,))
    m = _merge(engine, streams, ("f64",), tsm=range(k))
    rows, offs, ts, bits, vd = _per_column_merge(engine, m, 0)
    assert rows == m.out_rows
    assert (offs == m.offs).all()
    assert (ts == m.ts).all()
    assert (vd == m.valid[0]).all()
    assert (bits == m.bits[0]).all()
    _check(m, streams, ("f64",), nseries)
    _free(m)


def test_three_columns_independent_nulls(engine):
    r = np.random.default_rng(102)
    dtypes = ("f64",) * 3
    nseries = 2
    streams = _mk_streams(r, [2047, 2048, 2049, 5000], nseries, dtypes,
                          (0.0, 0.3, 0.9))
    m = _merge(engine, streams, dtypes, tsm=range(4))
    _check(m, streams, dtypes, nseries)
    for c in range(3):
        rows, offs, ts, bits, vd = _per_column_merge(engine, m, c)
        assert rows == m.out_rows and (offs == m.offs).all(), c
        assert (ts == m.ts).all(), c
        assert (vd == m.valid[c]).all(), c
        assert (bits == m.bits[c]).all(), c
    _free(m)


def test_mixed_widths_bit_blind(engine):
    r = np.random.default_rng(103)
    nseries = 2
    streams = _mk_streams(r, [2049, 5000, 2047], nseries, DTYPES,
                          (0.3, 0.3, 0.3, 0.3))
    # f64 column: NaNs with a distinct payload in every row
    serial = 1
    for f in range(3):
        for s in range(nseries):
            bits = streams[f][s][1][0][0]
            nan = r.random(bits.size) < 0.5
            pay = np.arange(serial, serial + bits.size, dtype=np.uint64)
            sign = np.where(r.random(bits.size) < 0.5,
                            np.uint64(1 << 63), np.uint64(0))
            bits[nan] = (np.uint64(0x7FF0000000000000) | sign | pay)[nan]
            serial += bits.size
    assert np.isnan(streams[0][0][1][0][0].view(np.float64)).any()
    assert (np.abs(streams[0][0][1][1][0].view(np.int64)) > (1 << 61)).all()
    assert (streams[0][0][1][2][0] > np.uint64(1 << 63)).all()
    m = _merge(engine, streams, DTYPES)
    _check(m, streams, DTYPES, nseries)  # bit-for-bit, nulls zero
    for c in range(4):
        assert (m.valid[c] == 0).any() and (m.valid[c] == 1).any()
    _free(m)


def test_absent_columns(engine):
    r = np.random.default_rng(104)
    dtypes = ("f64", "i64", "bool")
    nseries = 2
    # col 1 is absent in the two newest of four streams, col 2 everywhere
    absent = {(2, 1), (3, 1)} | {(f, 2) for f in range(4)}
    streams = _mk_streams(r, [2048, 5000, 2047, 2049], nseries, dtypes,
                          (0.3, 0.3, 0.0), absent)
    m = _merge(engine, streams, dtypes)
    _check(m, streams, dtypes, nseries)  # oracle: absent = all-null stream
    assert (m.valid[2] == 0).all() and (m.bits[2] == 0).all()
    _free(m)
    # d_valid NULL as a whole array: present columns are all-valid; output
    # validity entries of None are accepted
    m = _merge(engine, streams, dtypes, out_valid=False, drop_valid=True)
    assert all(v is None for v in m.valid)
    _check(m, streams, dtypes, nseries, all_valid=True)
    _free(m)


def test_raw_set_newest_stream(engine):
    """memcache rows (gs_raw_set) over 2 TSM streams, 2 columns"""
    r = np.random.default_rng(105)
    dtypes = ("f64", "f64")
    nseries = 3
    streams = _mk_streams(r, [2049, 2500, 700], nseries, dtypes, (0.3, 0.0))
    m = _merge(engine, streams, dtypes, tsm=(0, 1))
    _check(m, streams, dtypes, nseries)
    _free(m)


FUZZ_SEED = 2024
# (k, ncols) per trial: every k of {2, 5, 16} and ncols of {1, 2, 8, 32}
FUZZ_SHAPES = [(2, 2), (5, 8), (16, 32), (2, 32), (5, 1), (16, 8)]


def _fuzz_trial(r, k, ncols):
    nseries = int(r.integers(1, 4))
    sizes = [int(r.choice([1, 7, 2047, 2048, 2049, 5000])) for _ in range(k)]
    big = r.choice(k, size=2, replace=False)  # two streams of >= 2047 rows
    sizes[big[0]] = 5000
    sizes[big[1]] = int(r.choice([2047, 2048, 2049, 5000]))
    dtypes = tuple(DTYPES[int(i)] for i in r.integers(0, 4, ncols))
    null_rates = tuple(float(x) for x in r.choice([0.0, 0.3], ncols))
    absent = {(int(f), int(c))
              for f, c in zip(r.integers(0, k, (k * ncols) // 8),
                              r.integers(0, ncols, (k * ncols) // 8))}
    streams = _mk_streams(r, sizes, nseries, dtypes, null_rates, absent)
    return nseries, dtypes, null_rates, absent, streams


def _fuzz_walkback_stats(streams, nseries, dtypes, null_rates, absent):
    """Over the cells of null-carrying columns: (cells, cells whose value
    comes from a stream older than the newest one holding the timestamp,
    all-null cells)."""
    cells = older = nulls = 0
    for s in range(nseries):
        newest = _newest_holder(streams, s)
        for c in range(len(dtypes)):
            if not (null_rates[c] or any(ac == c for _, ac in absent)):
                continue
            _, sf, _, valid = _expect(streams, s, c)
            cells += valid.size
            older += int((valid & (sf < newest)).sum())
            nulls += int((~valid).sum())
    return cells, older, nulls


def test_fuzz(engine):
    r = np.random.default_rng(FUZZ_SEED)
    for trial, (k, ncols) in enumerate(FUZZ_SHAPES):
        nseries, dtypes, null_rates, absent, streams = _fuzz_trial(r, k, ncols)
        assert sum(len(st[0][0]) >= 2047 for st in streams) >= 2
        cells, older, nulls = _fuzz_walkback_stats(streams, nseries, dtypes,
                                                   null_rates, absent)
        if cells:  # the trial cannot pass without the walk-back
            assert older >= 0.01 * cells, (trial, older, cells)
            assert nulls >= 1, trial
        m = _merge(engine, streams, dtypes)
        _check(m, streams, dtypes, nseries, tag=f"trial {trial}")
        _free(m)


def test_merge_reencode_oracle_decode(engine):
    """merge -> GPU re-encode (ts + a null-carrying f64 column) -> oracle
    decode of the new pages == oracle merge"""
    r = np.random.default_rng(106)
    dtypes = ("f64", "i64")
    streams = _mk_streams(r, [1300, 1200, 1100], 1, dtypes, (0.3, 0.0))
    k = len(streams)
    gsets, tss, cols = [], [], []
    for f in range(k):
        g, t, cs = _upload_raw(engine, streams[f], dtypes)
        gsets.append(g)
        tss.append(t)
        cols.append(cs)
    total = sum(g.rows for g in gsets)
    d_ots = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_o0 = torch.zeros(total, dtype=torch.float64, device="cuda")
    d_v0 = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_o1 = torch.zeros(total, dtype=torch.int64, device="cuda")
    rows, offs = engine.compact_merge_fields(
        gsets, tss, cols, d_ots, [(d_o0, d_v0), (d_o1, None)])
    uts, sf, sj, valid = _expect(streams, 0, 0)
    assert rows == uts.size and 2900 < rows < 3600
    cap = rows * 12 + 128
    d_ets = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_ev = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    one = (np.array([0], dtype=np.int64), np.array([rows], dtype=np.int32))
    len_ts = engine.encode_pages_dev(0, d_ots, *one, d_ets, cap)[0]
    len_v = engine.encode_pages_dev(2, d_o0, *one, d_ev, cap, d_valid=d_v0)[0]
    pts = d_ets[:len_ts].cpu().numpy().tobytes()
    pv = d_ev[:len_v].cpu().numpy().tobytes()
    nb_t = int.from_bytes(pts[0:4], "big")
    nb_v = int.from_bytes(pv[0:4], "big")
    assert int.from_bytes(pts[4:12], "big") == rows
    assert int.from_bytes(pv[4:12], "big") == rows
    got_ts = orc.decode_i64(pts[16 + nb_t:], rows)
    got_valid = np.unpackbits(np.frombuffer(pv[16:16 + nb_v], dtype=np.uint8),
                              bitorder="little")[:rows].astype(bool)
    got_v = orc.decode_f64(pv[16 + nb_v:], rows, got_valid)
    assert (got_ts == uts).all()
    assert (got_valid == valid).all() and not valid.all()
    exp = _expected_bits(streams, 0, 0, "f64", sf, sj, valid)
    assert got_v.view(np.uint64)[valid].tolist() == exp[valid].tolist()
    for g in gsets:
        g.free()


def _tiny(engine, nseries=1, dtype=torch.float64, ncols=1, sorted_=True):
    counts = np.full(nseries, 4, dtype=np.int64)
    ts = np.tile(T0 + np.arange(4, dtype=np.int64) * NS, nseries)
    if not sorted_:
        ts[1], ts[2] = ts[2], ts[1]
    g = engine.raw_set(counts)
    d_ts = torch.from_numpy(ts).cuda()
    n = 4 * nseries
    cols = [(torch.arange(n, device="cuda").to(dtype), None)
            for _ in range(ncols)]
    return g, d_ts, cols, n


def _call(engine, parts, ncols=None, dtype=torch.float64):
    """compact_merge_fields over tiny streams; parts = [_tiny(...), ...]"""
    total = sum(p[3] for p in parts)
    ncols = len(parts[0][2]) if ncols is None else ncols
    d_ots = torch.zeros(total, dtype=torch.int64, device="cuda")
    outs = [(torch.zeros(total, dtype=dtype, device="cuda"), None)
            for _ in range(ncols)]
    rows, offs = engine.compact_merge_fields(
        [p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts],
        d_ots, outs)
    return rows, offs, d_ots, outs


def test_errors_leave_engine_usable(engine):
    good = [_tiny(engine), _tiny(engine)]

    def ok():
        rows, offs, d_ots, outs = _call(engine, good)
        assert rows == 4 and offs.tolist() == [0, 4]
        assert outs[0][0][:4].cpu().tolist() == [0.0, 1.0, 2.0, 3.0]

    ok()
    # unsorted stream: fails the way compact_merge fails
    bad = [_tiny(engine), _tiny(engine, sorted_=False)]
    total = 8
    with pytest.raises(RuntimeError) as e_old:
        engine.compact_merge(
            [p[0] for p in bad], [p[1] for p in bad],
            [p[2][0][0] for p in bad], [None, None],
            torch.zeros(total, dtype=torch.int64, device="cuda"),
            torch.zeros(total, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError) as e_new:
        _call(engine, bad)
    assert "(-3)" in str(e_old.value)  # GS_ERR_FORMAT
    assert str(e_new.value).split("(", 1)[1] == \
        str(e_old.value).split("(", 1)[1]  # same status, same message
    ok()
    # ncols = 33
    wide = [_tiny(engine, ncols=33), _tiny(engine, ncols=33)]
    with pytest.raises(RuntimeError, match=r"\(-1\).*ncols"):
        _call(engine, wide)
    ok()
    # elem_size 4
    i32 = [_tiny(engine, dtype=torch.int32), _tiny(engine, dtype=torch.int32)]
    with pytest.raises(RuntimeError, match=r"\(-1\).*elem_size"):
        _call(engine, i32, dtype=torch.int32)
    ok()
    # mismatched series counts
    mism = [_tiny(engine, nseries=1), _tiny(engine, nseries=2)]
    with pytest.raises(RuntimeError, match=r"\(-1\).*same series list"):
        _call(engine, mism)
    ok()
    for p in good + bad + wide + i32 + mism:
        p[0].free()
