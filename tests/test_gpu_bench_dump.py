"""bench.py end to end at a tiny shape: --steps/--warmup are honoured, the
result line carries ms_per_step, a plain run leaves the --full legs out,
and --dump-outputs writes the last timed step's outputs — identical from
run to run and bit-exact against the oracle's decode of the same pages."""
import json
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

NSERIES, NPTS, PAGE_ROWS, UNIQUE, STEPS, WARMUP = 8, 16000, 4000, 4, 2, 1
SHAPE = ["--series", str(NSERIES), "--npts", str(NPTS),
         "--page-rows", str(PAGE_ROWS), "--unique", str(UNIQUE)]


def _run(monkeypatch, capsys, extra):
    import bench
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", str(STEPS),
        "--warmup", str(WARMUP)] + SHAPE + extra)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_run_dumps_last_step_outputs(monkeypatch, capsys, tmp_path):
    import bench
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _run(monkeypatch, capsys, ["--dump-outputs", d1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0 and line["unit"] == "values/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] * line["ms_per_step"] / 1000
               - NSERIES * NPTS) < 1e-6 * NSERIES * NPTS
    # a plain run does not run the --full legs
    assert line["roofline"] is None and line["cpu_baseline"] is None
    a = _load(d1)
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6

    # same arguments -> same inputs -> same outputs
    _run(monkeypatch, capsys, ["--dump-outputs", d2])
    b = _load(d2)
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k

    # oracle: decode the same pages, closed-interval time filter, compact
    sub, _, npages = bench.build_workload(NSERIES, NPTS, PAGE_ROWS, UNIQUE, 2)
    lo, hi = int(0.25 * NPTS), int(0.75 * NPTS) - 1  # selected row span
    per_sb = NSERIES // 2
    nb = int(NPTS * bench.NS // bench.BUCKET_NS) + 1
    exp_cnt = np.zeros(nb, dtype=np.int64)
    exp_sum = np.zeros(nb)
    exp_max = np.full(nb, -np.inf)
    for sb, (buf, offs, lens, nvals, cts, sids) in enumerate(sub):
        raw = np.frombuffer(buf, np.uint8)
        ts_e, val_e = [], []
        for s in range(per_sb):
            v = []
            for p in range(npages):
                i = (s * npages + p) * 2 + 1  # [ts, val] per group
                pg = raw[offs[i]:offs[i] + lens[i]]
                hdr = int.from_bytes(pg[0:4].tobytes(), "big")
                v.append(orc.decode_f64(pg[16 + hdr:].tobytes(), PAGE_ROWS))
            v = np.concatenate(v)[lo:hi + 1]
            t = np.arange(lo, hi + 1, dtype=np.int64) * bench.NS
            ts_e.append(t)
            val_e.append(v)
            bi = t // bench.BUCKET_NS
            exp_cnt += np.bincount(bi, minlength=nb)
            exp_sum += np.bincount(bi, weights=v, minlength=nb)
            np.maximum.at(exp_max, bi, v)
        ts_e, val_e = np.concatenate(ts_e), np.concatenate(val_e)
        rows = a[f"buf{sb}_sample_rows"].astype(np.int64)
        assert rows.size == ts_e.size  # small output: dumped whole
        assert (a[f"buf{sb}_out_ts_minus_t0_ns"] == ts_e[rows]).all()
        assert (a[f"buf{sb}_out_val_f0"].view(np.uint64)
                == val_e[rows].view(np.uint64)).all()
    # the bucket aggregates accumulate over every step the run made
    nsteps = STEPS + WARMUP
    assert (a["agg_count"] == nsteps * exp_cnt).all()
    nz = exp_cnt > 0
    assert (a["agg_max"][nz] == exp_max[nz]).all()
    assert (a["agg_max"][~nz] == 0.0).all()  # empty buckets dumped as 0
    assert np.allclose(a["agg_sum"], nsteps * exp_sum, rtol=1e-12)


def test_full_run_keeps_roofline_and_cpu_baseline(monkeypatch, capsys):
    line = _run(monkeypatch, capsys, ["--full"])
    assert line["ms_per_step"] > 0 and line["steps"] == STEPS
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["frac"] > 0
    assert line["cpu_baseline"]["value"] > 0
    assert line["cpu_baseline"]["kind"] == "port"
    assert line["config"]["phase_ms_unoverlapped_per_subbatch"] is not None
