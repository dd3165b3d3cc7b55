#!/usr/bin/env python3
"""Times gs_compact_merge_fields against gs_compact_merge (since the fold of
the one-column kernel: the same kernel entered at ncols=1) on the
`bench.py --mode compact` shape (config #5: k=8 overlapping L0 streams per
series, each a random 25% subset of a shared grid) at a reduced series
count, and writes the figures as JSON.

Legs, interleaved per repeat so that drift hits all of them alike:
  a  gs_compact_merge once (one f64 column)
  b  gs_compact_merge_fields, ncols=1
  c  gs_compact_merge_fields, ncols=8, all-valid
  d  gs_compact_merge_fields, ncols=8, 10% nulls per column
  e  eight gs_compact_merge calls on the data of c (the per-column route)

Before timing, the ncols=8 result is compared with the per-column calls
(one kernel at ncols=8 and at ncols=1: a column does not depend on its
neighbours) and, for the first series, with the oracle's merge_dedup.

Each call is host-synchronous (it ends in a stream synchronize), so the
device events around it bracket the whole call: scratch allocation, the
three kernels and the offset round trip.

    python tools/compact_fields_probe.py --out profiles/compact_fields.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

T0 = 1_700_000_000_000_000_000
NS = 1_000_000_000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=128)
    ap.add_argument("--npts", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--ncols", type=int, default=8)
    ap.add_argument("--nulls", type=float, default=0.1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="profiles/compact_fields.json")
    args = ap.parse_args()

    import torch
    import cnosdb_amd as gs
    if not torch.cuda.is_available():
        sys.exit("compact_fields_probe needs a GPU: timings come from the "
                 "device only")
    eng = gs.Engine(0)
    rng = np.random.default_rng(231)
    k, nseries, ncols = args.k, args.series, args.ncols
    grid = T0 + np.arange(args.npts, dtype=np.int64) * NS
    gen = torch.Generator(device="cuda")
    gen.manual_seed(231)
    gsets, tss, vals, valids = [], [], [], []
    total = 0
    for f in range(k):
        ts = grid[rng.random(args.npts) < 0.25]
        gset = eng.raw_set(np.full(nseries, ts.size, dtype=np.int64))
        n = ts.size * nseries
        tss.append(torch.from_numpy(ts).cuda().repeat(nseries))
        vals.append([torch.rand(n, generator=gen, device="cuda",
                                dtype=torch.float64) for _ in range(ncols)])
        valids.append([(torch.rand(n, generator=gen, device="cuda")
                        >= args.nulls).to(torch.uint8) for _ in range(ncols)])
        gsets.append(gset)
        total += n
    d_ots = torch.zeros(total, dtype=torch.int64, device="cuda")
    outs = [(torch.zeros(total, dtype=torch.float64, device="cuda"),
             torch.zeros(total, dtype=torch.uint8, device="cuda"))
            for _ in range(ncols)]
    d_ots1 = torch.zeros(total, dtype=torch.int64, device="cuda")
    d_oval1 = torch.zeros(total, dtype=torch.float64, device="cuda")
    d_ovd1 = torch.zeros(total, dtype=torch.uint8, device="cuda")

    def fields(nc, with_nulls):
        cols = [[(vals[f][c], valids[f][c] if with_nulls else None)
                 for c in range(nc)] for f in range(k)]
        return eng.compact_merge_fields(gsets, tss, cols, d_ots, outs[:nc])[0]

    def single(c):
        return eng.compact_merge(gsets, tss, [vals[f][c] for f in range(k)],
                                 [None] * k, d_ots1, d_oval1, d_ovd1)[0]

    legs = {
        "a": ("gs_compact_merge x1", 1, lambda: single(0)),
        "b": ("gs_compact_merge_fields ncols=1", 1,
              lambda: fields(1, False)),
        "c": (f"gs_compact_merge_fields ncols={ncols} all-valid", ncols,
              lambda: fields(ncols, False)),
        "d": (f"gs_compact_merge_fields ncols={ncols} "
              f"{args.nulls:.0%} nulls per column", ncols,
              lambda: fields(ncols, True)),
        "e": (f"gs_compact_merge x{ncols}", ncols,
              lambda: [single(c) for c in range(ncols)][-1]),
    }

    # a column's result must not depend on its neighbours ...
    out_rows, offs = eng.compact_merge_fields(
        gsets, tss, [[(vals[f][c], None) for c in range(ncols)]
                     for f in range(k)], d_ots, outs)
    match = True
    for c in range(ncols):
        assert single(c) == out_rows
        match &= torch.equal(d_ots1[:out_rows], d_ots[:out_rows])
        match &= torch.equal(d_oval1[:out_rows].view(torch.int64),
                             outs[c][0][:out_rows].view(torch.int64))
    if not match:
        sys.exit("gs_compact_merge_fields differs from per-column "
                 "gs_compact_merge")
    # ... and must be the oracle's merge (first series, every column)
    from oracle import pyoracle as orc
    n0 = [int(t.numel()) // nseries for t in tss]
    hts = [t[:n].cpu().numpy() for t, n in zip(tss, n0)]
    lo, hi = int(offs[0]), int(offs[1])
    for c in range(ncols):
        uts, uval, _ = orc.merge_dedup(
            [(hts[f], vals[f][c][:n0[f]].cpu().numpy(), None)
             for f in range(k)])
        if not (np.array_equal(d_ots[lo:hi].cpu().numpy(), uts) and
                np.array_equal(outs[c][0][lo:hi].cpu().numpy().view(np.int64),
                               uval.view(np.int64))):
            sys.exit(f"gs_compact_merge_fields differs from the oracle "
                     f"merge in column {c}")

    ms = {name: [] for name in legs}
    for rep in range(args.warmup + args.repeats):
        for name, (_, _, fn) in legs.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))

    shape = (f"k={k} streams x {nseries} series, {args.npts}-point grid at "
             f"25% per stream, {total} rows in, {out_rows} rows out, f64")
    result = {"shape": shape, "rows_in": total, "rows_out": int(out_rows),
              "k": k, "series": nseries, "ncols": ncols,
              "null_rate_d": args.nulls, "warmup": args.warmup,
              "repeats": args.repeats,
              "device": torch.cuda.get_device_name(0),
              "timing": "device events around each host-synchronous call",
              "outputs_match_per_column_merge": True,
              "first_series_matches_oracle": True, "legs": {}}
    for name, (what, nc, _) in legs.items():
        med = statistics.median(ms[name])
        result["legs"][name] = {
            "what": what, "ms_median": med, "ms_min": min(ms[name]),
            "ms_max": max(ms[name]),
            "rows_in_per_s": total / (med / 1e3),
            "row_columns_in_per_s": total * nc / (med / 1e3),
        }
    m = {n: result["legs"][n]["ms_median"] for n in legs}
    result["ratios"] = {
        "e_over_c": m["e"] / m["c"],
        "b_over_a": m["b"] / m["a"],
        "d_minus_c_ms": m["d"] - m["c"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    for g in gsets:
        g.free()
    eng.close()


if __name__ == "__main__":
    main()
