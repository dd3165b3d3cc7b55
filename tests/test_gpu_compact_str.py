"""gs_compact_merge_group: the column-group merge with string columns.  A
string cell follows the rule of every other column
(BatchMergeBuilder::take_last_and_merge, reader/batch_builder.rs:132-155):
the newest stream that holds the timestamp, has the column and is valid
there wins, else the cell is null with length 0.

The expected winner per cell comes from orc.merge_dedup over an index
column (source-row ids, small integers, exact in float64); the expected
strings are the lookup.  The fixed-width columns of the same call must be
what compact_merge_fields gives on the same inputs, bit for bit."""
import numpy as np
import pytest
import torch

import cnosdb_amd as gs
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000_000_000_000
NS = 1_000_000_000
GRID = T0 + np.arange(6000, dtype=np.int64) * NS
STRIDE = 1 << 20
LENS = (0, 1, 7, 8, 9, 15, 16, 17, 300)
GS_ERR, GS_ERR_CAP = -1, -5
POISON = 0x5A


@pytest.fixture(scope="module")
def engine():
    e = gs.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------ data

class _Stream:
    """One stream: per series ts, fixed columns [(array, valid|None)] and
    string columns [(list of bytes, valid|None) or None = absent]."""

    def __init__(self, series):
        self.series = series


def _strings(r, n):
    out = []
    for ln in r.choice(LENS, n):
        out.append(bytes(r.integers(0x21, 0x7f, ln, dtype=np.uint8)))
    return out


def _mk(seed, sizes, str_spec, fixed=True):
    """sizes[f][s] rows; str_spec[c] = (streams that have column c, null
    rate or None for d_valid NULL)."""
    r = np.random.default_rng(seed)
    streams = []
    for f, per in enumerate(sizes):
        series = []
        for n in per:
            ts = GRID[np.sort(r.choice(GRID.size, size=n, replace=False))]
            fx = []
            if fixed:
                fx = [(np.round(r.normal(50, 10, n), 1), r.random(n) >= 0.3),
                      (np.round(r.normal(5, 1, n), 2), None),
                      (r.integers(0, 2, n, dtype=np.uint8),
                       r.random(n) >= 0.2)]
            sc = []
            for present, rate in str_spec:
                if f not in present:
                    sc.append(None)
                else:
                    sc.append((_strings(r, n),
                               None if rate is None else r.random(n) >= rate))
            series.append((ts, fx, sc))
        streams.append(_Stream(series))
    return streams


def _upload(engine, st, null_fill=3):
    """Raw set + device columns of one stream.  Null string rows own
    null_fill bytes of 0xEE that must never come out."""
    counts = np.array([t.size for t, _, _ in st.series], dtype=np.int64)
    gset = engine.raw_set(counts)
    d_ts = torch.from_numpy(
        np.concatenate([t for t, _, _ in st.series])).cuda()
    nfx = len(st.series[0][1])
    cols = []
    for c in range(nfx):
        v = np.concatenate([fx[c][0] for _, fx, _ in st.series])
        d_vd = None
        if st.series[0][1][c][1] is not None:
            d_vd = torch.from_numpy(np.concatenate(
                [fx[c][1] for _, fx, _ in st.series]).astype(np.uint8)).cuda()
        cols.append((torch.from_numpy(v).cuda(), d_vd))
    scols = []
    for c in range(len(st.series[0][2])):
        if st.series[0][2][c] is None:
            scols.append(None)
            continue
        parts, valid, has_valid = [], [], st.series[0][2][c][1] is not None
        for _, _, sc in st.series:
            strs, vd = sc[c]
            for j, s in enumerate(strs):
                ok = vd is None or vd[j]
                parts.append(s if ok else b"\xEE" * null_fill)
                valid.append(ok)
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        data = np.frombuffer(b"".join(parts) + b"\0", np.uint8).copy()
        scols.append((torch.from_numpy(off).cuda(),
                      torch.from_numpy(data).cuda(),
                      torch.from_numpy(np.array(valid, np.uint8)).cuda()
                      if has_valid else None))
    return gset, d_ts, cols, scols


def _expect_strings(streams, c):
    """Merged column c over all series: bytes or None per output row."""
    out = []
    for s in range(len(streams[0].series)):
        per = []
        for f, st in enumerate(streams):
            ts, _, sc = st.series[s]
            ids = (f * STRIDE + np.arange(ts.size)).astype(np.float64)
            if sc[c] is None:
                valid = np.zeros(ts.size, bool)
            else:
                valid = sc[c][1]
            per.append((ts, ids, valid))
        _, ids, valid = orc.merge_dedup(per)
        ids = ids.astype(np.int64)
        for i, ok in zip(ids, valid):
            out.append(streams[i // STRIDE].series[s][2][c][0][i % STRIDE]
                       if ok else None)
    return out


class _Run:
    pass


def _merge(engine, streams, caps=None, out_valid=True):
    ups = [_upload(engine, st) for st in streams]
    gsets = [u[0] for u in ups]
    total = sum(g.rows for g in gsets)
    nfx, nstr = len(ups[0][2]), len(ups[0][3])
    d_ots = torch.zeros(total, dtype=torch.int64, device="cuda")

    def fixed_outs():
        outs = []
        for c in range(nfx):
            dt = ups[0][2][c][0].dtype
            if dt == torch.uint8:
                d_v = torch.full((total,), POISON, dtype=dt, device="cuda")
            else:
                d_v = torch.full((total,), 0x5A5A5A5A5A5A5A5A,
                                 dtype=torch.int64, device="cuda").view(dt)
            outs.append((d_v, torch.full((total,), POISON, dtype=torch.uint8,
                                         device="cuda")))
        return outs

    run = _Run()
    run.gsets, run.total, run.nstr = gsets, total, nstr
    expect = [_expect_strings(streams, c) for c in range(nstr)]
    run.expect = expect
    exact = [sum(len(s) for s in e if s is not None) for e in expect]
    run.exact = exact
    caps = exact if caps is None else caps
    outs = fixed_outs()
    souts = [(torch.full((total + 1,), -1, dtype=torch.int64, device="cuda"),
              torch.full((max(caps[c], 1),), POISON, dtype=torch.uint8,
                         device="cuda")[:caps[c]],
              torch.full((total,), POISON, dtype=torch.uint8, device="cuda")
              if out_valid else None) for c in range(nstr)]
    run.souts = souts
    try:
        run.out_rows, run.offs, run.totals = engine.compact_merge_group(
            gsets, [u[1] for u in ups], [u[2] for u in ups],
            [u[3] for u in ups], d_ots, outs, souts)
    except RuntimeError:
        for c in range(nstr):  # a failed call writes no string bytes
            assert bool((souts[c][1] == POISON).all())
        _free(run)
        raise
    run.ts = d_ots[:run.out_rows].cpu().numpy()
    run.fixed = [(v[:run.out_rows].cpu().numpy(),
                  vd[:run.out_rows].cpu().numpy()) for v, vd in outs]
    if nfx:
        ref = fixed_outs()
        d_rts = torch.zeros(total, dtype=torch.int64, device="cuda")
        run.ref_rows, run.ref_offs = engine.compact_merge_fields(
            gsets, [u[1] for u in ups], [u[2] for u in ups], d_rts, ref)
        run.ref_ts = d_rts[:run.ref_rows].cpu().numpy()
        run.ref_fixed = [(v[:run.ref_rows].cpu().numpy(),
                          vd[:run.ref_rows].cpu().numpy()) for v, vd in ref]
    return run


def _check_strings(run):
    n = run.out_rows
    for c in range(run.nstr):
        exp = run.expect[c]
        assert len(exp) == n
        off = np.zeros(n + 1, np.int64)
        np.cumsum([len(s) if s is not None else 0 for s in exp], out=off[1:])
        d_off, d_bytes, d_vd = run.souts[c]
        assert run.totals[c] == int(off[-1]) == run.exact[c]
        assert (d_off[:n + 1].cpu().numpy() == off).all()
        got = d_bytes[:run.totals[c]].cpu().numpy().tobytes()
        assert got == b"".join(s for s in exp if s is not None)
        if d_vd is not None:
            assert (d_vd[:n].cpu().numpy() ==
                    np.array([s is not None for s in exp], np.uint8)).all()


def _check_fixed(run):
    assert run.out_rows == run.ref_rows
    assert (run.offs == run.ref_offs).all()
    assert (run.ts == run.ref_ts).all()
    for (v, vd), (rv, rvd) in zip(run.fixed, run.ref_fixed):
        assert v.tobytes() == rv.tobytes()
        assert (vd == rvd).all()


def _free(run):
    for g in run.gsets:
        g.free()


# column A: absent in the oldest stream, 30 % nulls; column B: present in
# stream 1 only, passed with d_valid NULL
SPEC = [({1, 2}, 0.3), ({1}, None)]
SIZES = [[0, 1, 2047, 2048, 2049], [7, 0, 1500, 1500, 1500],
         [3, 2, 1500, 900, 1]]


# ----------------------------------------------------------------- tests

def test_mixed_group_tile_and_scan_seams(engine):
    streams = _mk(1, SIZES, SPEC)
    run = _merge(engine, streams)
    try:
        assert run.out_rows > 4096 + 2048  # several scan blocks
        _check_fixed(run)
        _check_strings(run)
        # what the data must contain for the claims above
        a = run.expect[0]
        assert any(s is None for s in a) and any(s == b"" for s in a)
        assert {len(s) for s in a if s is not None} >= set(LENS)
    finally:
        _free(run)


def test_newer_null_does_not_hide_older_value_and_all_null_cell(engine):
    """Three one-series streams over the same four timestamps."""
    ts = GRID[:4].copy()
    mk = lambda strs, valid: _Stream([(ts, [], [(strs, np.array(valid))])])
    streams = [mk([b"old0", b"old1", b"old2", b"old3"], [1, 1, 0, 1]),
               mk([b"mid0", b"mid1", b"mid2", b"mid3"], [1, 0, 0, 1]),
               mk([b"new0", b"new1", b"new2", b""], [1, 0, 0, 1])]
    run = _merge(engine, streams)
    try:
        assert run.expect[0] == [b"new0", b"old1", None, b""]
        assert (run.ts == ts).all()
        _check_strings(run)
    finally:
        _free(run)


def test_without_output_validity(engine):
    streams = _mk(2, [[300], [200], [250]], SPEC, fixed=False)
    run = _merge(engine, streams, out_valid=False)
    try:
        _check_strings(run)
    finally:
        _free(run)


def test_nstr_0_is_compact_merge_fields(engine):
    streams = _mk(3, [[700, 2100], [650, 10], [900, 2049]], [])
    run = _merge(engine, streams)
    try:
        assert run.nstr == 0 and run.totals == []
        _check_fixed(run)
    finally:
        _free(run)


def test_bytes_cap_exact_and_one_short(engine):
    streams = _mk(4, [[400], [300], [350]], SPEC)
    run = _merge(engine, streams)  # caps = the exact totals
    try:
        _check_strings(run)
        exact = run.exact
    finally:
        _free(run)
    assert exact[0] > 0
    with pytest.raises(RuntimeError) as ei:
        _merge(engine, streams, caps=[exact[0] - 1, exact[1]])
    assert ei.value.status == GS_ERR_CAP
    assert ei.value.total_bytes == exact
    # the context is usable, and roomy buffers are fine too
    run = _merge(engine, streams, caps=[exact[0] + 64, exact[1] + 1])
    try:
        _check_strings(run)
    finally:
        _free(run)


def test_33_columns_is_gs_err(engine):
    n = 8
    ts = GRID[:n].copy()
    fx = [(np.arange(n, dtype=np.float64), None)] * 32
    sc = [([b"x"] * n, None)]
    streams = [_Stream([(ts, fx, sc)]), _Stream([(ts, fx, sc)])]
    with pytest.raises(RuntimeError, match=r"\(-1\).*ncols \+ nstr") as ei:
        _merge(engine, streams)
    assert ei.value.status == GS_ERR
    # 31 + 1 is the limit and works
    for st in streams:
        st.series = [(ts, fx[:31], sc)]
    run = _merge(engine, streams)
    try:
        _check_fixed(run)
        _check_strings(run)
    finally:
        _free(run)


@pytest.mark.parametrize("cap_blocks", [1, 3])
def test_past_the_grid(engine, cap_blocks):
    streams = _mk(5, [[900, 2100, 5], [800, 40, 0], [850, 2060, 9]], SPEC)
    with gs.grid_cap(cap_blocks):
        run = _merge(engine, streams)
        assert gs.grid_rounds() > 1
    try:
        _check_fixed(run)
        _check_strings(run)
    finally:
        _free(run)


def test_merge_encode_upload_decode(engine):
    """End to end: the merged column goes through encode_str_pages_dev as
    it is, and the pages decode to the expectation."""
    streams = _mk(6, [[500], [450], [480]], [({0, 1, 2}, 0.25)], fixed=False)
    run = _merge(engine, streams)
    try:
        n = run.out_rows
        exp = run.expect[0]
        d_off, d_bytes, d_vd = run.souts[0]
        sizes = [1000] * (n // 1000) + ([n % 1000] if n % 1000 else [])
        row_off = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        pay = [sum(len(s) + (2 if len(s) > 127 else 1)
                   for s in exp[o:o + m] if s is not None)
               for o, m in zip(row_off, sizes)]
        cap = max(16 + (m + 7) // 8 + 34 + p + p // 6
                  for m, p in zip(sizes, pay))
        d_out = torch.zeros(len(sizes) * cap, dtype=torch.uint8, device="cuda")
        info = engine.encode_str_pages_dev(d_off, d_bytes, row_off, sizes,
                                           d_out, cap, d_vd)
        out = d_out.cpu().numpy()
        groups = []
        for p, m in enumerate(sizes):
            page = out[p * cap:p * cap + int(info["len"][p])].tobytes()
            assert page == gs.str_page_of(
                [s or b"" for s in exp[row_off[p]:row_off[p] + m]],
                [s is not None for s in exp[row_off[p]:row_off[p] + m]])
            tsp = run.ts[row_off[p]:row_off[p] + m]
            groups.append((p, [(gs.page_of(tsp, gs.CT_TIME), gs.CT_TIME),
                               (page, gs.CT_STR)]))
        gset = engine.upload(groups)
        try:
            total = run.totals[0]
            r_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
            r_bytes = torch.zeros(max(total, 1), dtype=torch.uint8,
                                  device="cuda")
            r_vd = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
            assert engine.decode_str(gset, 1, r_off, r_bytes, r_vd) == total
            assert torch.equal(r_off, d_off[:n + 1])
            assert torch.equal(r_bytes[:total], d_bytes[:total])
            assert torch.equal(r_vd, d_vd[:n])
        finally:
            gset.free()
    finally:
        _free(run)
