"""Fused decode+aggregate (k_gor_chunks_filtered<AGG> + k_agg_fixup): the
bucket max/sum/count accumulated inside the Gorilla decode kernel against a
numpy composition of the oracle's decode of the same pages.

Count and max are exact, sum within rtol=1e-12, two identical runs are
bit-identical, and the fused path agrees with GS_AGG_FUSED=0 (today's
separate aggregate pass) — the knob is read once per process, so the two
settings run in fresh child processes that execute the same cases.

Shapes are the smallest that still reach every piece rule: 4500-row pages
give chunks of 2048/2048/404 rows (head, complete and tail pieces in one
chunk), 100-row pages make a 300-row bucket out of four or more head/tail
pieces across pages."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = 1_700_000_000 * NS
HERE = os.path.abspath(__file__)


def _values(rng, n):
    return np.round(np.clip(np.cumsum(rng.normal(0, 0.5, n)) + 50, 0, 100), 1)


def _nan_values(rng, n):
    v = _values(rng, n)
    v[n // 3:n // 3 + 700] = 100.0          # a run of the clip ceiling
    nan = np.array([0x7FF8000000000123], dtype=np.uint64).view(np.float64)[0]
    v[5::997] = nan                          # NaN payloads, several buckets
    v[n // 3 + 10] = nan                     # ... one inside the 100.0 run
    return v


# name -> (page row counts of one series, nseries, nfields, value maker,
#          [(time range in rows (lo, hi) or None for an empty range,
#            bucket seconds, t0 offset seconds from T0, n_buckets), ...])
# Rows are 1 s apart (but see SPACING), so rows and seconds are
# interchangeable below.
CASES = {
    # bucket edges at rows = 37 mod 300: never on a chunk edge (2048, 4096,
    # 4500, 6548, ...) nor a page edge; range starts/ends mid-bucket and
    # mid-chunk
    "pages4500": ([4500] * 3, 3, 1, _values,
                  [((1111, 12345), 300, -263, 47)]),
    # one chunk per page: every bucket is made of head/tail pieces only
    "pages100": ([100] * 7, 3, 1, _values,
                 [((0, 699), 300, -50, 4), ((130, 555), 300, -50, 4)]),
    # a bucket exactly one chunk long on the chunk grid, and one longer
    # than a whole series
    "chunk_bucket": ([4500] * 2, 2, 1, _values,
                     [((0, 8999), 2048, 0, 5), ((100, 8000), 2048, 0, 5),
                      ((0, 8999), 1_000_000, -17, 1)]),
    # t0 later than the first selected rows, n_buckets too small for the
    # last ones
    "grid_edges": ([4500] * 2, 2, 1, _values,
                   [((1000, 8500), 300, 2500, 10)]),
    # nothing selected, then everything, then a part: no stale cells
    "empty_full": ([4500] * 2, 2, 1, _values,
                   [(None, 300, -263, 32), ((0, 8999), 300, -263, 32),
                    ((3000, 3100), 300, -263, 32)]),
    # 1-row buckets: below the gate (2 rows per bucket), so the separate
    # aggregate pass runs; 5-row buckets: fused, ~400 complete pieces per
    # chunk
    "small_buckets": ([4500], 2, 1, _values,
                      [((7, 4321), 1, -3, 4504), ((7, 4321), 5, -3, 902)]),
    # two fields, odd total_rows: field 1 starts at an odd row
    "two_fields_odd": ([4500, 4501], 3, 2, _values,
                       [((1111, 8123), 300, -263, 32)]),
    "nan_100": ([4500] * 2, 2, 1, _nan_values,
                [((50, 8900), 300, -263, 32)]),
    # series 0 at 1 s, series 1 at 10 s (SPACING): 5 s buckets pass the gate
    # on the set's smallest delta, and on series 1 every other bucket is an
    # empty complete cell between two rows
    "mixed_spacing": ([4500], 2, 1, _values,
                      [((7, 40000), 5, -3, 8002)]),
}
SPACING = {"mixed_spacing": [1, 10]}  # seconds per row, by series; default 1


def _build(name):
    """Pages of one case + the oracle's decode of those very pages."""
    import cnosdb_amd as gs
    from oracle import pyoracle as orc

    page_rows, nseries, nf, mk, _ = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    groups, truth = [], []

    def data_of(pg, n, dec):
        pg = np.frombuffer(pg, np.uint8)
        hdr = int.from_bytes(pg[0:4].tobytes(), "big")
        return dec(pg[16 + hdr:].tobytes(), n)

    for s in range(nseries):
        n_all = sum(page_rows)
        step = SPACING.get(name, [1])
        ts = T0 + np.arange(n_all, dtype=np.int64) * NS * step[s % len(step)]
        vals = [mk(rng, n_all) for _ in range(nf)]
        dts, dvals, r0 = [], [[] for _ in range(nf)], 0
        for n in page_rows:
            tp = gs.page_of(ts[r0:r0 + n], gs.CT_TIME)
            pages = [(tp, gs.CT_TIME)]
            dts.append(data_of(tp, n, orc.decode_i64))
            for f in range(nf):
                vp = gs.page_of(vals[f][r0:r0 + n], gs.CT_F64)
                pages.append((vp, gs.CT_F64))
                dvals[f].append(data_of(vp, n, orc.decode_f64))
            groups.append((s, pages))
            r0 += n
        truth.append((np.concatenate(dts),
                      [np.concatenate(v) for v in dvals]))
    return groups, truth


def _expect(truth, nf, lo, hi, t0, bucket_ns, nb):
    """numpy composition: closed-range filter, compaction, bucket agg with
    the engine's max rule (x > mx: a NaN never wins, the sum carries it)."""
    out_ts, out_val = [], [[] for _ in range(nf)]
    mx = np.full((nf, nb), -np.inf)
    sm = np.zeros((nf, nb))
    ct = np.zeros((nf, nb), dtype=np.int64)
    for ts, vals in truth:
        s = np.searchsorted(ts, lo, side="left")
        e = np.searchsorted(ts, hi, side="right")
        t = ts[s:e]
        out_ts.append(t)
        b = (t - t0) // bucket_ns
        m = (b >= 0) & (b < nb)
        for f in range(nf):
            v = vals[f][s:e]
            out_val[f].append(v)
            np.add.at(ct[f], b[m], 1)
            ssum = np.zeros(nb)
            np.add.at(ssum, b[m], v[m])
            sm[f] += ssum
            ok = m & ~np.isnan(v)
            np.maximum.at(mx[f], b[ok], v[ok])
    return (np.concatenate(out_ts),
            [np.concatenate(v) for v in out_val], mx, sm, ct)


def _scan(eng, gset, nf, lo, hi, t0, bucket_ns, nb):
    import torch
    import cnosdb_amd as gs
    rows = gset.rows
    d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
    d_ots = torch.zeros(rows, dtype=torch.int64, device="cuda")
    d_oval = torch.zeros(nf * rows, dtype=torch.float64, device="cuda")
    agg = dict(bucket_ns=bucket_ns, t0=t0, n_buckets=nb,
               d_max=torch.full((nf * nb,), -np.inf, dtype=torch.float64,
                                device="cuda"),
               d_sum=torch.zeros(nf * nb, dtype=torch.float64, device="cuda"),
               d_count=torch.zeros(nf * nb, dtype=torch.int64, device="cuda"))
    if nf == 1:
        res = eng.scan(gset, d_ts, d_val, time_range=(lo, hi),
                       d_out_ts=d_ots, d_out_val=d_oval, agg=agg)
    else:
        res = gs.scan_fields(eng, gset, list(range(nf)), d_ts, d_val,
                             (lo, hi), d_ots, d_oval, agg=agg)
    n = int(res.out_rows)
    return dict(
        ts=d_ots[:n].cpu().numpy(),
        val=np.stack([d_oval[f * rows:f * rows + n].cpu().numpy()
                      for f in range(nf)]),
        mx=agg["d_max"].cpu().numpy().reshape(nf, nb),
        sm=agg["d_sum"].cpu().numpy().reshape(nf, nb),
        ct=agg["d_count"].cpu().numpy().reshape(nf, nb))


def _queries(name):
    for rng_rows, bucket_s, t0_off, nb in CASES[name][4]:
        if rng_rows is None:
            lo, hi = T0 - 500 * NS, T0 - 100 * NS
        else:
            # closed range that starts and ends between two rows
            lo = T0 + rng_rows[0] * NS - NS // 2
            hi = T0 + rng_rows[1] * NS + NS // 3
        yield lo, hi, T0 + t0_off * NS, bucket_s * NS, nb


def _run_case(eng, name):
    """All queries of a case on ONE uploaded set, in order (the stale-cell
    cases depend on it); each query runs twice."""
    groups, truth = _build(name)
    nf = CASES[name][2]
    gset = eng.upload(groups)
    got = []
    try:
        for q in _queries(name):
            a = _scan(eng, gset, nf, *q)
            b = _scan(eng, gset, nf, *q)
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (name, k)
            got.append(a)
    finally:
        gset.free()
    return truth, got


def _same_sum(got, exp, what):
    nan = np.isnan(exp)
    assert (np.isnan(got) == nan).all(), what
    err = np.abs(got[~nan] - exp[~nan])
    tol = 1e-12 * np.abs(exp[~nan])
    print(what, "max rel sum err",
          float((err / np.maximum(np.abs(exp[~nan]), 1e-300)).max())
          if err.size else 0.0)
    assert (err <= tol).all(), what


@pytest.fixture(scope="module")
def engine():
    import cnosdb_amd as gs
    e = gs.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", list(CASES))
def test_fused_agg_matches_oracle(engine, name):
    truth, got = _run_case(engine, name)
    nf = CASES[name][2]
    for qi, (q, g) in enumerate(zip(_queries(name), got)):
        ets, evals, emx, esm, ect = _expect(truth, nf, *q)
        what = f"{name}[{qi}]"
        assert (g["ts"] == ets).all(), what
        for f in range(nf):
            assert (g["val"][f].view(np.uint64)
                    == evals[f].view(np.uint64)).all(), what
        assert (g["ct"] == ect).all(), what
        assert (g["mx"].view(np.uint64) == emx.view(np.uint64)).all(), what
        _same_sum(g["sm"], esm, what)
    if name == "empty_full":
        assert (got[0]["ct"] == 0).all() and np.isinf(got[0]["mx"]).all()
    if name == "nan_100":
        assert np.isnan(got[0]["sm"]).any() and (got[0]["mx"] == 100.0).any()


def _child(path):
    import torch
    # torch brings the HIP runtime up first, as under pytest (conftest)
    assert torch.cuda.is_available(), "child needs a GPU"
    import cnosdb_amd as gs
    eng = gs.Engine(0)
    out = {}
    for name in CASES:
        _, got = _run_case(eng, name)
        for qi, g in enumerate(got):
            for k, v in g.items():
                out[f"{name}.{qi}.{k}"] = v
    eng.close()
    np.savez(path, **out)


def test_fused_and_separate_paths_agree(tmp_path):
    res = {}
    for knob in ("0", "1"):
        path = str(tmp_path / f"agg{knob}.npz")
        env = dict(os.environ, GS_AGG_FUSED=knob)
        subprocess.run([sys.executable, HERE, path], check=True, env=env,
                       cwd=os.path.dirname(os.path.dirname(HERE)),
                       timeout=300)
        res[knob] = np.load(path)
    assert sorted(res["0"].files) == sorted(res["1"].files)
    for k in res["0"].files:
        a, b = res["0"][k], res["1"][k]
        if k.endswith(".sm"):
            _same_sum(b, a, k)
        else:  # compacted ts/values, count, max: bit-identical
            assert a.tobytes() == b.tobytes(), k


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    _child(sys.argv[1])
