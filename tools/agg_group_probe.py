#!/usr/bin/env python3
"""Times gs_agg_group against gs_filter_group projecting the same columns,
which is the least a caller had to run before aggregating elsewhere, and
writes the figures as JSON.  The first shape is the set of
tools/filter_group_probe.py (series x 4k-row pages, 10% nulls, two tombstone
ranges, v > 50, the middle half of the time line), so the figures line up
with profiles/filter_group.json; two more shapes over the same decoded
columns stress the split of the row space:

  tsbs         the page set, one bucket per page span (series x pages cells)
  few_long     4 series of rows / 4 rows, one bucket each: a cell runs over
               tens of thousands of wave segments
  many_short   series of 1..64 rows, two buckets each: every wave step
               holds several cells

Legs per shape, interleaved per repeat so that drift hits all alike:
  f1_parent, f8_parent   gs_filter_group of a parent checkout given with
                         --parent, 1 and 8 projected f64 columns
  f1, f8                 the same on this tree
  g1, g8                 gs_agg_group, 1 and 8 aggregated f64 columns, all
                         six aggregates, and d_rows
All times are device events around the kernels of one call
(cnosdb_amd.filter_ms / agg_ms).

Before timing, the kept rows of g1 must add up to f1's out_rows, its sums to
the sum of f1's output column, and on the page set a sample of series is
held to tests/agg_ref.py.

    python tools/agg_group_probe.py --parent ../parent \
        --out profiles/agg_group.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from filter_group_probe import NS, T0, load_package  # noqa: E402

SIX = ("count", "sum", "min", "max", "first", "last")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=2500)
    ap.add_argument("--npts", type=int, default=40_000)
    ap.add_argument("--page-rows", type=int, default=4000)
    ap.add_argument("--unique", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent", default=None,
                    help="a built checkout of the parent commit")
    ap.add_argument("--out", default="profiles/agg_group.json")
    args = ap.parse_args()

    import torch
    import cnosdb_amd as gs
    import agg_ref as ar
    import filter_ref as fr
    if not torch.cuda.is_available():
        sys.exit("agg_group_probe needs a GPU: timings come from the device "
                 "only")
    rng = np.random.default_rng(231)
    nseries, npts, page_rows = args.series, args.npts, args.page_rows
    npages = npts // page_rows
    uniq = min(args.unique, nseries)
    tpages = [gs.page_of(
        T0 + (np.arange(page_rows, dtype=np.int64) + p * page_rows) * NS,
        gs.CT_TIME) for p in range(npages)]
    vpool = []
    for _ in range(uniq):
        walk = np.round(np.clip(
            np.cumsum(rng.normal(0, 0.5, page_rows)) + 50, 0, 100), 1)
        vpool.append(gs.page_of(walk, gs.CT_F64,
                                rng.random(page_rows) > 0.10))
    groups = [(s, [(tpages[p], gs.CT_TIME),
                   (vpool[(s * npages + p) % uniq], gs.CT_F64)])
              for s in range(nseries) for p in range(npages)]
    eng = gs.Engine(0)
    gset = eng.upload(groups)
    rows = gset.rows
    parent = peng = None
    if args.parent:
        parent = load_package(os.path.abspath(args.parent),
                              "cnosdb_amd_parent")
        assert not hasattr(parent.Engine, "agg_group"), \
            "--parent is not the parent commit"
        peng = parent.Engine(0)

    # decoded once, outside the timed region
    d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
    d_vd = torch.zeros(rows, dtype=torch.uint8, device="cuda")
    eng.decode(gset, 0, d_ts)
    eng.decode(gset, 1, d_val, d_vd)
    f_in = [(d_val, d_vd)] + [(torch.roll(d_val, 7 * c), torch.roll(d_vd, 7 * c))
                              for c in range(1, 8)]
    o_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    f_out = [(torch.zeros(rows, dtype=torch.float64, device="cuda"),
              torch.zeros(rows, dtype=torch.uint8, device="cuda"))
             for _ in range(8)]
    p1 = [(0, "gt", 50.0)]

    def line(sizes):
        """Timestamps of a raw set: one row per second from T0 in every
        series."""
        sz = torch.from_numpy(np.asarray(sizes, np.int64)).cuda()
        start = torch.cumsum(sz, 0) - sz
        idx = torch.arange(rows, dtype=torch.int64, device="cuda")
        return T0 + (idx - torch.repeat_interleave(start, sz)) * NS

    def window(n):
        """The middle half of a line of n points and two tombstone ranges,
        placed as on the page set."""
        return ((T0 + int(0.25 * n) * NS, T0 + int(0.75 * n) * NS - 1),
                [(T0 + int(0.30 * n) * NS, T0 + int(0.33 * n) * NS - 1),
                 (T0 + int(0.60 * n) * NS, T0 + int(0.63 * n) * NS - 1)])

    long_sizes = [rows // 4] * 3 + [rows - 3 * (rows // 4)]
    short_sizes = rng.integers(1, 65, rows // 32 + 64)
    short_sizes = short_sizes[np.cumsum(short_sizes) <= rows]
    short_sizes = np.append(short_sizes, rows - short_sizes.sum())
    short_sizes = short_sizes[short_sizes > 0]
    shapes = {
        "tsbs": dict(what=f"{nseries} series x {npages} pages of {page_rows} "
                          "rows, one bucket per page span",
                     sets=(gset, peng.upload(groups) if peng else None),
                     ts=d_ts, win=window(npts), nseries=nseries,
                     bucket_ns=page_rows * NS, n_buckets=npages),
        "few_long": dict(what="4 series, one bucket each",
                         sets=(eng.raw_set(long_sizes),
                               peng.raw_set(long_sizes) if peng else None),
                         ts=line(long_sizes), win=window(rows // 4),
                         nseries=4, bucket_ns=0, n_buckets=1),
        "many_short": dict(what="series of 1..64 rows, two buckets of 32 s",
                           sets=(eng.raw_set(short_sizes),
                                 peng.raw_set(short_sizes) if peng else None),
                           ts=line(short_sizes), win=((T0 + 2 * NS,
                                                       T0 + 60 * NS),
                                                      [(T0 + 20 * NS,
                                                        T0 + 21 * NS)]),
                           nseries=len(short_sizes), bucket_ns=32 * NS,
                           n_buckets=2),
    }

    result = {
        "rows": rows, "warmup": args.warmup, "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0),
        "filter_tile": gs.filter_tile(),
        "timing": "device events from the first to the last kernel of one "
                  "call; f*: gs_filter_group projecting the columns, g*: "
                  "gs_agg_group aggregating them (count, sum, min, max, "
                  "first, last, and d_rows)",
        "bar": "median(g) <= median(f_parent) + (max - min)(f_parent), the "
               "parent's gs_filter_group on the same inputs projecting the "
               "same columns",
        "shapes": {}}

    for sname, sh in shapes.items():
        here, pset = sh["sets"]
        ts, (rng_t, tstones) = sh["ts"], sh["win"]
        ncell = sh["nseries"] * sh["n_buckets"]
        outs = [{n: torch.zeros(ncell, dtype=torch.int64, device="cuda")
                 for n in SIX} for _ in range(8)]
        d_rows = torch.zeros(ncell, dtype=torch.int64, device="cuda")

        def fcols(nf, tstones=tstones):
            return [(gs.CT_F64, f_in[c][0], f_in[c][1],
                     tstones if c == 0 else [], f_out[c][0], f_out[c][1])
                    for c in range(nf)]

        def filt(e, s, pkg, nf, ts=ts, rng_t=rng_t):
            out_rows, _ = e.filter_group(s, ts, fcols(nf), p1, (),
                                         time_range=rng_t, d_out_ts=o_ts)
            return pkg.filter_ms(), int(out_rows)

        def agg(nf, ts=ts, rng_t=rng_t, here=here, sh=sh, outs=outs,
                d_rows=d_rows):
            eng.agg_group(here, ts, fcols(nf), p1,
                          [(c, outs[c]) for c in range(nf)], T0,
                          sh["bucket_ns"], sh["n_buckets"], True,
                          time_range=rng_t, d_rows=d_rows)
            return gs.agg_ms(), int(d_rows.sum())

        legs = {"f1": lambda: filt(eng, here, gs, 1),
                "f8": lambda: filt(eng, here, gs, 8),
                "g1": lambda: agg(1), "g8": lambda: agg(8)}
        if peng:
            legs = dict({"f1_parent": lambda: filt(peng, pset, parent, 1),
                         "f8_parent": lambda: filt(peng, pset, parent, 8)},
                        **legs)

        # ---- outputs first
        _, kept = legs["f1"]()
        f_sum = float(f_out[0][0][:kept].sum())
        _, g_rows = legs["g1"]()
        if g_rows != kept:
            sys.exit(f"{sname}: gs_agg_group keeps {g_rows} rows, "
                     f"gs_filter_group {kept}")
        g_sum = float(outs[0]["sum"].view(torch.float64).sum())
        if abs(g_sum - f_sum) > 1e-9 * abs(f_sum):
            sys.exit(f"{sname}: sums differ: {g_sum} against {f_sum}")
        sample = []
        if sname == "tsbs":
            sample = sorted({0, 1, nseries // 2, nseries - 1})
            for s in sample:
                sl = slice(s * npts, (s + 1) * npts)
                case = fr.Case(f"series {s}", [npts], ts[sl].cpu().numpy(),
                               [fr.Col(fr.CT_F64, f_in[0][0][sl].cpu().numpy(),
                                       f_in[0][1][sl].cpu().numpy(), tstones)],
                               [], p1, rng_t)
                ref = ar.agg_ref(ar.AggCase(case, [(0, SIX)], T0,
                                            sh["bucket_ns"], sh["n_buckets"],
                                            True))
                cells = slice(s * npages, (s + 1) * npages)
                ok = d_rows[cells].cpu().tolist() == ref["rows"]
                for n in SIX:
                    got = outs[0][n][cells].cpu().numpy().view(np.uint64)
                    for i in range(npages):
                        w = ref["cols"][0]
                        same = (ar.sum_within(fr.CT_F64, int(got[i]),
                                              w["sum"][i], w["count"][i],
                                              w["sum_abs"][i])
                                if n == "sum" else
                                int(got[i]) == w[n][i] & ar.M64)
                        ok = ok and same
                if not ok:
                    sys.exit(f"tsbs, series {s}: differs from agg_ref")

        # ---- timing
        ms = {n: [] for n in legs}
        for rep in range(args.warmup + args.repeats):
            for n, run in legs.items():
                t, _ = run()
                if rep >= args.warmup:
                    ms[n].append(t)
        res = {"what": sh["what"], "series": sh["nseries"], "cells": ncell,
               "rows_kept": kept, "sample_series_match_agg_ref": sample,
               "legs": {n: {"ms_median": statistics.median(v),
                            "ms_min": min(v), "ms_max": max(v),
                            "spread_ms": max(v) - min(v)}
                        for n, v in ms.items()}}
        for nf in (1, 8):
            g = res["legs"][f"g{nf}"]
            base = res["legs"].get(f"f{nf}_parent")
            if base:
                res[f"bar_{nf}_columns"] = {
                    "g_ms": g["ms_median"], "f_parent_ms": base["ms_median"],
                    "ratio": g["ms_median"] / base["ms_median"],
                    "f_parent_spread_ms": base["spread_ms"],
                    "g_spread_ms": g["spread_ms"],
                    "holds": bool(g["ms_median"] <= base["ms_median"] +
                                  base["spread_ms"])}
            else:
                res[f"bar_{nf}_columns"] = ("not measured: no --parent "
                                            "checkout given")
        result["shapes"][sname] = res
        if sname != "tsbs":
            here.free()
            if pset:
                pset.free()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    gset.free()
    eng.close()


if __name__ == "__main__":
    main()
