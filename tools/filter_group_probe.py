#!/usr/bin/env python3
"""Times gs_filter_group against gs_scan's general path (k_vmask +
k_compact_masked) on the `bench.py --mode general` shape (series x 4k-row
pages, 10% nulls, two tombstone ranges, v > 50, the middle half of the time
line) at a reduced point count, and writes the figures as JSON.  The set is
decoded once outside the timed region.

Legs, interleaved per repeat so that drift hits all of them alike:
  a_parent  gs_scan of a parent checkout given with --parent (its package
            is loaded beside this tree's, in the same process)
  a         gs_scan on this tree; both: ms_filter + ms_compact of
            GsScanResult (device events; the decode phases are excluded)
  b         gs_filter_group, the same predicate, tombstones and range, one
            projected f64 column
  c         the same predicate with 8 projected f64 columns
  d         two predicates on two columns, projecting 8 f64 + 1 bool +
            1 string column (8-byte strings)
b, c and d: device events around the kernels of one call
(cnosdb_amd.filter_ms), and the host-synchronous wall time beside them.

Before timing, b must give gs_scan's rows, and a sample of groups of every
leg is held to tests/filter_ref.py.

    python tools/filter_group_probe.py --parent ../parent \
        --out profiles/filter_group.json
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

T0 = 1_700_000_000_000_000_000
NS = 1_000_000_000
# MI355X: plain coalesced stores 6.0-6.2 TB/s, achievable HBM about 6.3 TB/s
PLAIN_STORE_BPS = 6.0e12


def load_package(path, name):
    """A second checkout's cnosdb_amd under another module name."""
    init = os.path.join(path, "cnosdb_amd", "__init__.py")
    spec = importlib.util.spec_from_file_location(
        name, init, submodule_search_locations=[os.path.dirname(init)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


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
    ap.add_argument("--out", default="profiles/filter_group.json")
    args = ap.parse_args()

    import torch
    import cnosdb_amd as gs
    import filter_ref as fr
    if not torch.cuda.is_available():
        sys.exit("filter_group_probe needs a GPU: timings come from the "
                 "device only")
    rng = np.random.default_rng(231)
    nseries, npts, page_rows = args.series, args.npts, args.page_rows
    npages = npts // page_rows
    lo = T0 + int(0.25 * npts) * NS
    hi = T0 + int(0.75 * npts) * NS - 1
    tstones = [(T0 + int(0.30 * npts) * NS, T0 + int(0.33 * npts) * NS - 1),
               (T0 + int(0.60 * npts) * NS, T0 + int(0.63 * npts) * NS - 1)]
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

    def scan_leg(pkg):
        eng = pkg.Engine(0)
        gset = eng.upload(groups)
        n = gset.rows
        bufs = [torch.zeros(n, dtype=dt, device="cuda") for dt in
                (torch.int64, torch.float64, torch.int64, torch.float64)]

        def run():
            r = eng.scan(gset, bufs[0], bufs[1], time_range=(lo, hi),
                         tombstones=tstones, d_out_ts=bufs[2],
                         d_out_val=bufs[3], value_pred=("gt", 50.0))
            return r.ms_filter + r.ms_compact, int(r.out_rows)
        return eng, gset, bufs, run

    eng, gset, sbufs, scan_here = scan_leg(gs)
    rows = gset.rows
    parent_run = None
    if args.parent:
        parent = load_package(os.path.abspath(args.parent),
                              "cnosdb_amd_parent")
        assert not hasattr(parent.Engine, "filter_group"), \
            "--parent is not the parent commit"
        _, pset, pbufs, parent_run = scan_leg(parent)

    # decoded once, outside the timed region
    d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
    d_vd = torch.zeros(rows, dtype=torch.uint8, device="cuda")
    eng.decode(gset, 0, d_ts)
    eng.decode(gset, 1, d_val, d_vd)
    f_in = [(d_val, d_vd)] + [(torch.roll(d_val, 7 * c), torch.roll(d_vd, 7 * c))
                              for c in range(1, 8)]
    b_in = ((d_val > 50).to(torch.uint8), d_vd)
    s_off = torch.arange(rows + 1, dtype=torch.int64, device="cuda") * 8
    s_bytes = torch.randint(0x21, 0x7f, (rows * 8,), dtype=torch.uint8,
                            device="cuda")
    o_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    f_out = [(torch.zeros(rows, dtype=torch.float64, device="cuda"),
              torch.zeros(rows, dtype=torch.uint8, device="cuda"))
             for _ in range(8)]
    b_out = (torch.zeros(rows, dtype=torch.uint8, device="cuda"),
             torch.zeros(rows, dtype=torch.uint8, device="cuda"))
    s_out = (torch.zeros(rows + 1, dtype=torch.int64, device="cuda"),
             torch.zeros(rows * 8, dtype=torch.uint8, device="cuda"),
             torch.zeros(rows, dtype=torch.uint8, device="cuda"))

    def fcols(nf):
        return [(gs.CT_F64, f_in[c][0], f_in[c][1], tstones if c == 0 else [],
                 f_out[c][0], f_out[c][1]) for c in range(nf)]

    def filt(cols, preds, strs=()):
        t0 = time.perf_counter()
        out_rows, offs = eng.filter_group(gset, d_ts, cols, preds, strs,
                                          time_range=(lo, hi), d_out_ts=o_ts)
        wall = (time.perf_counter() - t0) * 1e3
        return gs.filter_ms(), int(out_rows), wall, offs

    p1 = [(0, "gt", 50.0)]
    legs = {
        "b": ("gs_filter_group, 1 predicate, 1 projected f64", 1, 1,
              lambda: filt(fcols(1), p1)),
        "c": ("gs_filter_group, 1 predicate, 8 projected f64", 1, 8,
              lambda: filt(fcols(8), p1)),
        "d": ("gs_filter_group, 2 predicates on 2 columns, 8 f64 + 1 bool "
              "+ 1 string projected", 2, 10,
              lambda: filt(fcols(8) + [(gs.CT_BOOL, b_in[0], b_in[1], [],
                                        b_out[0], b_out[1])],
                           p1 + [(1, "lt", 80.0)],
                           [((s_off, s_bytes, None), [], s_out)])),
    }

    # ---- outputs first: b is gs_scan's, a sample of groups is filter_ref's
    _, scan_rows = scan_here()
    _, b_rows, _, _ = legs["b"][3]()
    same = (b_rows == scan_rows and
            torch.equal(o_ts[:b_rows], sbufs[2][:b_rows]) and
            torch.equal(f_out[0][0][:b_rows].view(torch.int64),
                        sbufs[3][:b_rows].view(torch.int64)))
    if not same:
        sys.exit("gs_filter_group differs from gs_scan")
    if parent_run and parent_run()[1] != scan_rows:
        sys.exit("the parent's gs_scan selects other rows")
    sample = sorted({0, 1, 2, gset.ngroups // 2, gset.ngroups - 1})
    h_ts = d_ts.cpu().numpy().reshape(-1, page_rows)
    for name in legs:
        _, out_rows, _, offs = legs[name][3]()
        nf = legs[name][2] if name != "d" else 8
        for g in sample:
            sl = slice(g * page_rows, (g + 1) * page_rows)
            cols = [fr.Col(fr.CT_F64, f_in[c][0][sl].cpu().numpy(),
                           f_in[c][1][sl].cpu().numpy(),
                           tstones if c == 0 else []) for c in range(nf)]
            preds = p1 if name != "d" else p1 + [(1, "lt", 80.0)]
            ref = fr.filter_ref(fr.Case(name, [page_rows], h_ts[g], cols, [],
                                        preds, (lo, hi)))
            a, b = int(offs[g]), int(offs[g + 1])
            ok = b - a == ref.out_rows and np.array_equal(
                o_ts[a:b].cpu().numpy(), ref.ts)
            for c in range(nf):
                ok = ok and np.array_equal(
                    f_out[c][0][a:b].cpu().numpy().view(np.uint8),
                    ref.cols[c][0])
                ok = ok and np.array_equal(f_out[c][1][a:b].cpu().numpy(),
                                           ref.cols[c][1])
            if not ok:
                sys.exit(f"leg {name}, group {g}: differs from filter_ref")

    # ---- timing
    names = (["a_parent"] if parent_run else []) + ["a"] + list(legs)
    ms = {n: [] for n in names}
    wall = {n: [] for n in legs}
    kept = {}
    for rep in range(args.warmup + args.repeats):
        for n in names:
            if n == "a_parent":
                t, r = parent_run()
            elif n == "a":
                t, r = scan_here()
            else:
                t, r, w, _ = legs[n][3]()
                if rep >= args.warmup:
                    wall[n].append(w)
            kept[n] = r
            if rep >= args.warmup:
                ms[n].append(t)

    def stats(v):
        return {"ms_median": statistics.median(v), "ms_min": min(v),
                "ms_max": max(v)}

    result = {
        "shape": f"{nseries} series x {npages} pages of {page_rows} rows, "
                 f"{rows} rows, 10% nulls, 2 tombstone ranges, v > 50, the "
                 f"middle half of the time line",
        "rows": rows, "groups": gset.ngroups, "warmup": args.warmup,
        "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
        "filter_tile": gs.filter_tile(),
        "timing": "a: GsScanResult.ms_filter + ms_compact; b-d: device "
                  "events from the first to the last kernel of the call; "
                  "wall_ms: host clock around the host-synchronous call",
        "b_equals_gs_scan": True, "sample_groups_match_filter_ref": sample,
        "legs": {}}
    what = {"a_parent": "gs_scan on the parent commit",
            "a": "gs_scan on this tree"}
    for n in names:
        leg = dict(what=what.get(n) or legs[n][0], rows_out=kept[n],
                   **stats(ms[n]))
        if n in legs:
            leg["wall_ms_median"] = statistics.median(wall[n])
            npred, nproj = legs[n][1], legs[n][2]
            k = kept[n]
            # mask: ts + per predicate value and validity, mask out; gather:
            # mask in, per kept row ts in/out and per column value and
            # validity in/out (strings: 8 B reference, length pass, bytes)
            moved = rows * (8 + 9 * npred + 1) + rows + k * 16
            nfix8 = min(nproj, 8)
            moved += k * nfix8 * 18
            if n == "d":
                moved += k * 4 + k * (9 + 8 + 8 + 8 + 8 + 16)
            leg["bytes_moved"] = moved
            leg["bytes_per_s"] = moved / (leg["ms_median"] / 1e3)
            leg["share_of_plain_store_rate"] = (leg["bytes_per_s"] /
                                                PLAIN_STORE_BPS)
        result["legs"][n] = leg
    base = result["legs"].get("a_parent")
    if base:
        width = base["ms_max"] - base["ms_min"]
        b = result["legs"]["b"]["ms_median"]
        result["rule"] = {
            "what": "median(b) <= median(a_parent) + (max - min)(a_parent)",
            "b_ms": b, "a_parent_ms": base["ms_median"],
            "a_parent_width_ms": width,
            "holds": bool(b <= base["ms_median"] + width)}
    else:
        result["rule"] = "not measured: no --parent checkout given"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    gset.free()
    eng.close()


if __name__ == "__main__":
    main()
