#!/usr/bin/env python3
"""Times gs_encode_group_pages_dev against the per-column routes (since the
fold of the one-column kernel, gs_encode_pages_dev is the same two kernels
entered with one column), on the merged output of the compact_fields_probe
shape (k=8 overlapping L0 streams per series, each a random 25% subset of a
shared grid), split into 1000-row blocks per series, and writes the figures
as JSON.

Legs, interleaved per repeat so that drift hits all of them alike:
  a_new  ts + one all-valid f64: one gs_encode_group_pages_dev call
  a_old  the same through two gs_encode_pages_dev calls (ts, f64)
  b_new  ts + 8 columns (f64, i64, u64, bool mixed, nulls): one call
  b_old  the only route without the new entry: ts and the f64 columns
         through gs_encode_pages_dev, every other column copied
         device-to-host and encoded there page by page with page_of

Every call is host-synchronous, so the device events around a leg bracket
all of it, host work included.  b_old also reports its copy time (host
clock around the synchronous copies).  Before timing, every page the group
call emits is compared with the per-column routes' pages (the same kernels
with other neighbours) and with the host encoder's page (page_of), which is
what says that the bytes are right.

    python tools/encode_group_probe.py --out profiles/encode_group.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

T0 = 1_700_000_000_000_000_000
NS = 1_000_000_000
MIX = ("f64", "i64", "u64", "bool", "f64", "i64", "u64", "bool")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=128)
    ap.add_argument("--npts", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--nulls", type=float, default=0.1)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="profiles/encode_group.json")
    args = ap.parse_args()

    import torch
    import cnosdb_amd as gs
    if not torch.cuda.is_available():
        sys.exit("encode_group_probe needs a GPU: timings come from the "
                 "device only")
    eng = gs.Engine(0)
    rng = np.random.default_rng(231)
    k, nseries, ncols = args.k, args.series, len(MIX)
    CT = {"f64": gs.CT_F64, "i64": gs.CT_I64, "u64": gs.CT_U64,
          "bool": gs.CT_BOOL}
    TD = {"f64": torch.float64, "i64": torch.int64, "u64": torch.int64,
          "bool": torch.uint8}
    grid = T0 + np.arange(args.npts, dtype=np.int64) * NS
    gen = torch.Generator(device="cuda")
    gen.manual_seed(231)

    def values(dt, n):
        if dt == "f64":  # one decimal, like a gauge
            return torch.round(torch.rand(n, generator=gen, device="cuda",
                                          dtype=torch.float64) * 1000) / 10
        if dt == "bool":
            return torch.randint(0, 2, (n,), generator=gen, device="cuda",
                                 dtype=torch.uint8)
        v = torch.randint(-1000, 1000, (n,), generator=gen, device="cuda",
                          dtype=torch.int64)
        return v + (-(1 << 63) if dt == "u64" else 0)  # u64 bits around 2^63

    gsets, tss, cols, total = [], [], [], 0
    for f in range(k):
        ts = grid[rng.random(args.npts) < 0.25]
        n = ts.size * nseries
        gsets.append(eng.raw_set(np.full(nseries, ts.size, dtype=np.int64)))
        tss.append(torch.from_numpy(ts).cuda().repeat(nseries))
        cols.append([(values(dt, n),
                      (torch.rand(n, generator=gen, device="cuda")
                       >= args.nulls).to(torch.uint8)) for dt in MIX])
        total += n
    d_ts = torch.zeros(total, dtype=torch.int64, device="cuda")
    merged = [(torch.zeros(total, dtype=TD[dt], device="cuda"),
               torch.zeros(total, dtype=torch.uint8, device="cuda"))
              for dt in MIX]
    out_rows, offs = eng.compact_merge_fields(gsets, tss, cols, d_ts, merged)
    # leg a's column: the first f64 column merged without its nulls
    d_allvalid = torch.zeros(total, dtype=torch.float64, device="cuda")
    eng.compact_merge_fields(gsets, tss, [[(c[0][0], None)] for c in cols],
                             torch.zeros_like(d_ts), [(d_allvalid, None)])
    for g in gsets:
        g.free()
    del cols, tss

    row_off, rows = [], []
    for s in range(nseries):
        r = int(offs[s])
        while r < offs[s + 1]:
            n = min(args.block_rows, int(offs[s + 1]) - r)
            row_off.append(r)
            rows.append(n)
            r += n
    row_off = np.array(row_off, dtype=np.int64)
    rows = np.array(rows, dtype=np.int32)
    npages, br = rows.size, args.block_rows
    bl = (br + 7) // 8
    cap_int = 16 + bl + 2 + 8 * br + 32
    cap_f64 = 16 + bl + 2 + 8 + (br + 1) * 10 + 16
    cap_bool = 16 + bl + 2 + 10 + bl
    CAP = {"f64": cap_f64, "i64": cap_int, "u64": cap_int, "bool": cap_bool}

    def outbuf(cap):
        return torch.zeros(npages * cap, dtype=torch.uint8, device="cuda")

    new_ts, new_cols = outbuf(cap_int), [outbuf(CAP[dt]) for dt in MIX]
    old_ts, old_cols = outbuf(cap_int), [outbuf(CAP[dt]) for dt in MIX]
    host_pages = {}  # b_old's host-encoded pages of the last run
    copy_s = []

    def a_new():
        return eng.encode_group_pages_dev(
            [(gs.CT_TIME, d_ts, None), (gs.CT_F64, d_allvalid, None)],
            row_off, rows, [(new_ts, cap_int), (new_cols[0], cap_f64)])

    def a_old():
        return (eng.encode_pages_dev(0, d_ts, row_off, rows, old_ts, cap_int),
                eng.encode_pages_dev(2, d_allvalid, row_off, rows,
                                     old_cols[0], cap_f64))

    def b_new():
        return eng.encode_group_pages_dev(
            [(gs.CT_TIME, d_ts, None)] +
            [(CT[dt], v, vd) for dt, (v, vd) in zip(MIX, merged)],
            row_off, rows,
            [(new_ts, cap_int)] + [(o, CAP[dt])
                                   for dt, o in zip(MIX, new_cols)])

    def b_old():
        lens = {"ts": eng.encode_pages_dev(0, d_ts, row_off, rows, old_ts,
                                           cap_int)}
        spent = 0.0
        for c, (dt, (v, vd)) in enumerate(zip(MIX, merged)):
            if dt == "f64":
                lens[c] = eng.encode_pages_dev(2, v, row_off, rows,
                                               old_cols[c], cap_f64,
                                               d_valid=vd)
                continue
            t0 = time.perf_counter()
            hv = v[:out_rows].cpu().numpy()
            hvd = vd[:out_rows].cpu().numpy().astype(bool)
            spent += time.perf_counter() - t0
            if dt == "u64":
                hv = hv.view(np.uint64)
            host_pages[c] = [
                gs.page_of(hv[o:o + n], CT[dt], hvd[o:o + n])
                for o, n in zip(row_off, rows)]
        copy_s.append(spent)
        return lens

    # ---- the new call must emit the pages the old routes emit
    def cut(buf, cap, lens):
        h = buf.cpu().numpy()
        return [h[p * cap:p * cap + int(lens[p])].tobytes()
                for p in range(npages)]

    def host(v, ct, vd=None):  # the host encoder's pages of a device column
        hv = v[:out_rows].cpu().numpy()
        hvd = None if vd is None else vd[:out_rows].cpu().numpy().astype(bool)
        return [gs.page_of(hv[o:o + n], ct,
                           None if hvd is None else hvd[o:o + n])
                for o, n in zip(row_off, rows)]

    ia, (lt, lf) = a_new(), a_old()
    same = cut(new_ts, cap_int, ia[0]["len"]) == cut(old_ts, cap_int, lt)
    same &= cut(new_cols[0], cap_f64, ia[1]["len"]) == \
        cut(old_cols[0], cap_f64, lf)
    right = cut(new_ts, cap_int, ia[0]["len"]) == host(d_ts, gs.CT_TIME)
    right &= cut(new_cols[0], cap_f64, ia[1]["len"]) == \
        host(d_allvalid, gs.CT_F64)
    ib, lb = b_new(), b_old()
    same &= cut(new_ts, cap_int, ib[0]["len"]) == cut(old_ts, cap_int, lb["ts"])
    for c, dt in enumerate(MIX):
        got = cut(new_cols[c], CAP[dt], ib[1 + c]["len"])
        exp = cut(old_cols[c], cap_f64, lb[c]) if dt == "f64" \
            else host_pages[c]
        same &= got == exp
    if not same:
        sys.exit("gs_encode_group_pages_dev pages differ from the old routes")
    for c, dt in enumerate(MIX):
        if dt == "f64":
            right &= cut(new_cols[c], cap_f64, ib[1 + c]["len"]) == \
                host(merged[c][0], gs.CT_F64, merged[c][1])
    if not right:
        sys.exit("device pages differ from the host encoder's pages")
    null_cells = sum(int(i["null_count"].sum()) for i in ib[1:])
    copy_s.clear()

    legs = {"a_new": a_new, "a_old": a_old, "b_new": b_new, "b_old": b_old}
    ms = {name: [] for name in legs}
    for rep in range(args.warmup + args.repeats):
        for name, fn in legs.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    copy_ms = [s * 1e3 for s in copy_s[args.warmup:]]

    what = {
        "a_new": "ts + all-valid f64: gs_encode_group_pages_dev x1",
        "a_old": "ts + all-valid f64: gs_encode_pages_dev x2",
        "b_new": f"ts + {ncols} mixed columns, {args.nulls:.0%} nulls per "
                 "input column: gs_encode_group_pages_dev x1",
        "b_old": f"ts + {ncols} mixed columns: gs_encode_pages_dev for ts and "
                 "f64, device-to-host copy + page_of per page for the rest",
    }
    result = {
        "shape": f"merged output of k={k} streams x {nseries} series, "
                 f"{args.npts}-point grid at 25% per stream: {int(out_rows)} "
                 f"rows, {npages} pages of <= {br} rows per column",
        "rows": int(out_rows), "pages_per_column": int(npages),
        "block_rows": br, "columns_b": ["ts"] + list(MIX),
        "null_cells_b": null_cells,
        "null_cell_share_b": null_cells / (int(out_rows) * ncols),
        "warmup": args.warmup, "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0),
        "timing": "device events around each host-synchronous leg",
        "pages_match_old_routes": True, "pages_match_host_encoder": True,
        "legs": {}}
    for name in legs:
        med = statistics.median(ms[name])
        nc = 2 if name[0] == "a" else 1 + ncols
        result["legs"][name] = {
            "what": what[name], "ms_median": med, "ms_min": min(ms[name]),
            "ms_max": max(ms[name]),
            "row_columns_per_s": int(out_rows) * nc / (med / 1e3)}
    result["legs"]["b_old"]["copy_ms_median"] = statistics.median(copy_ms)
    result["legs"]["b_old"]["copy_ms_min"] = min(copy_ms)
    result["legs"]["b_old"]["copy_ms_max"] = max(copy_ms)
    m = {n: result["legs"][n]["ms_median"] for n in legs}
    result["ratios"] = {
        "a_new_over_a_old": m["a_new"] / m["a_old"],
        "b_old_over_b_new": m["b_old"] / m["b_new"],
        "b_old_copy_share": statistics.median(copy_ms) / m["b_old"],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    eng.close()


if __name__ == "__main__":
    main()
