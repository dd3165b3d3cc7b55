#!/usr/bin/env python3
"""Times the string side of device compaction and writes the figures as
JSON: gs_compact_merge_group with string columns, and
gs_encode_str_pages_dev against the route it replaces.

Shape: the compact_fields_probe shape (k=8 overlapping L0 streams per
series, each a random 25% subset of a shared grid, 8 f64 columns), plus a
tag-like string column (a few hundred distinct values of 8-24 bytes) and a
high-entropy string column (random bytes, 8-24 each); the merged output is
split into pages of at most 1000 rows per series.

Merge legs (interleaved per repeat so that drift hits all of them alike):
  m_fields  gs_compact_merge_fields, 8 f64 columns
  m_group0  gs_compact_merge_group, the same 8 columns, nstr = 0
            (the same kernels: must agree within the legs' own spread)
  m_group1  + the tag column
  m_group2  + both string columns
Encode legs, per string column:
  e_dev     gs_encode_str_pages_dev
  e_host    the route without it: offsets, bytes and validity copied to the
            host (reported separately), then gs_encode_str + gs_build_page
            per page over the host copy, single-threaded as that entry is

Every call is host-synchronous, so the device events around a leg bracket
all of it, host work included.  Each timed call follows an untimed call of
the same leg: the host legs idle the device for half a second, and the leg
behind them would otherwise pay for the clocks coming back up.  Before
timing, every page the device encodes is compared with the oracle's block
under the page layout.

    python tools/str_compact_probe.py --out profiles/str_compact.json
"""
import argparse
import ctypes
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", type=int, default=128)
    ap.add_argument("--npts", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--nulls", type=float, default=0.1)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="profiles/str_compact.json")
    args = ap.parse_args()

    import torch
    import cnosdb_amd as gs
    from oracle import pyoracle as orc
    if not torch.cuda.is_available():
        sys.exit("str_compact_probe needs a GPU: timings come from the "
                 "device only")
    eng = gs.Engine(0)
    lib = gs.PageLib().lib
    rng = np.random.default_rng(231)
    k, nseries, nf64 = args.k, args.series, 8
    grid = T0 + np.arange(args.npts, dtype=np.int64) * NS
    gen = torch.Generator(device="cuda")
    gen.manual_seed(231)

    # the tag dictionary: 300 values of 8..24 bytes, padded to 24
    ntags = 300
    tag_len = torch.from_numpy(rng.integers(8, 25, ntags)).cuda()
    tag_bytes = torch.from_numpy(
        rng.integers(0x61, 0x7b, (ntags, 24), dtype=np.uint8)).cuda()

    def str_column(n, tags):
        """(offsets, bytes, valid) of n strings on the device."""
        if tags:
            ids = torch.randint(0, ntags, (n,), generator=gen, device="cuda")
            lens = tag_len[ids]
        else:
            lens = torch.randint(8, 25, (n,), generator=gen, device="cuda")
        off = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=off[1:])
        total = int(off[-1])
        if tags:
            row = torch.repeat_interleave(
                torch.arange(n, device="cuda"), lens)
            pos = torch.arange(total, device="cuda") - off[row]
            data = tag_bytes[ids[row], pos]
        else:
            data = torch.randint(0, 256, (total,), generator=gen,
                                 device="cuda", dtype=torch.uint8)
        valid = (torch.rand(n, generator=gen, device="cuda")
                 >= args.nulls).to(torch.uint8)
        return off, data.contiguous(), valid

    gsets, tss, cols, scols, total = [], [], [], [], 0
    for f in range(k):
        ts = grid[rng.random(args.npts) < 0.25]
        n = ts.size * nseries
        gsets.append(eng.raw_set(np.full(nseries, ts.size, dtype=np.int64)))
        tss.append(torch.from_numpy(ts).cuda().repeat(nseries))
        cols.append([(torch.round(torch.rand(n, generator=gen, device="cuda",
                                             dtype=torch.float64) * 1000) / 10,
                      (torch.rand(n, generator=gen, device="cuda")
                       >= args.nulls).to(torch.uint8)) for _ in range(nf64)])
        scols.append([str_column(n, True), str_column(n, False)])
        total += n
    in_bytes = [sum(int(sc[c][0][-1]) for sc in scols) for c in range(2)]

    d_ts = torch.zeros(total, dtype=torch.int64, device="cuda")
    merged = [(torch.zeros(total, dtype=torch.float64, device="cuda"),
               torch.zeros(total, dtype=torch.uint8, device="cuda"))
              for _ in range(nf64)]
    souts = [(torch.zeros(total + 1, dtype=torch.int64, device="cuda"),
              torch.zeros(in_bytes[c], dtype=torch.uint8, device="cuda"),
              torch.zeros(total, dtype=torch.uint8, device="cuda"))
             for c in range(2)]

    def m_fields():
        return eng.compact_merge_fields(gsets, tss, cols, d_ts, merged)

    def m_group(nstr):
        return eng.compact_merge_group(
            gsets, tss, cols, [sc[:nstr] for sc in scols], d_ts, merged,
            souts[:nstr])

    out_rows, offs, totals = m_group(2)

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
    worst = br * 25  # 24 bytes and a length byte per string
    cap = 16 + (br + 7) // 8 + 2 + 32 + worst + worst // 6
    d_pages = torch.zeros(npages * cap, dtype=torch.uint8, device="cuda")
    copy_s = {0: [], 1: []}
    host_buf = np.zeros(cap, dtype=np.uint8)
    page_buf = np.zeros(cap, dtype=np.uint8)

    def ptr(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def e_dev(c):
        d_off, d_bytes, d_vd = souts[c]
        return eng.encode_str_pages_dev(d_off, d_bytes, row_off, rows,
                                        d_pages, cap, d_vd)

    def host_columns(c):
        d_off, d_bytes, d_vd = souts[c]
        return (d_off[:out_rows + 1].cpu().numpy(),
                d_bytes[:totals[c]].cpu().numpy(),
                d_vd[:out_rows].cpu().numpy())

    def host_page(off, data, vd, o, n, encode):
        """One page through `encode` (gs_encode_str or the oracle's) and
        gs_build_page, from host arrays, without Python string objects."""
        v = vd[o:o + n] != 0
        lens = (off[o + 1:o + n + 1] - off[o:o + n])[v].astype(np.uint64)
        # null rows are zero-length in a merged column: the bytes of the
        # page's valid strings lie back to back
        src = data[off[o]:off[o + n]]
        if src.size == 0:
            src = np.zeros(1, np.uint8)
        dl = encode(ptr(src), ptr(lens), ctypes.c_int64(lens.size),
                    ptr(host_buf),
                    ctypes.c_size_t(host_buf.size)) if lens.size else 0
        bits = np.packbits(v, bitorder="little")
        pl = lib.gs_build_page(ptr(bits), ctypes.c_int64(n), ptr(host_buf),
                               ctypes.c_size_t(dl), ptr(page_buf),
                               ctypes.c_size_t(page_buf.size))
        return page_buf[:pl].tobytes()

    def e_host(c):
        t0 = time.perf_counter()
        off, data, vd = host_columns(c)
        copy_s[c].append(time.perf_counter() - t0)
        for o, n in zip(row_off, rows):
            host_page(off, data, vd, int(o), int(n), lib.gs_encode_str)

    # ---- every device page against the oracle's encoder
    olib = orc.Oracle().lib
    olib.orc_str_encode.restype = ctypes.c_int64
    for c in range(2):
        info = e_dev(c)
        h = d_pages.cpu().numpy()
        off, data, vd = host_columns(c)
        for p, (o, n) in enumerate(zip(row_off, rows)):
            got = h[p * cap:p * cap + int(info["len"][p])].tobytes()
            if got != host_page(off, data, vd, int(o), int(n),
                                olib.orc_str_encode):
                sys.exit(f"string column {c}, page {p}: device page differs "
                         "from the oracle's")
    for c in copy_s:
        copy_s[c].clear()

    legs = {"m_fields": m_fields, "m_group0": lambda: m_group(0),
            "m_group1": lambda: m_group(1), "m_group2": lambda: m_group(2),
            "e_dev_tags": lambda: e_dev(0), "e_host_tags": lambda: e_host(0),
            "e_dev_random": lambda: e_dev(1),
            "e_host_random": lambda: e_host(1)}
    ms = {name: [] for name in legs}
    for rep in range(args.warmup + args.repeats):
        for name, fn in legs.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            fn()  # untimed: no leg inherits its predecessor's clocks
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))

    result = {
        "shape": f"k={k} streams x {nseries} series, {args.npts}-point grid "
                 f"at 25% per stream, {nf64} f64 columns + a tag-like and a "
                 f"high-entropy string column (8-24 bytes), "
                 f"{args.nulls:.0%} nulls per input column: {int(out_rows)} "
                 f"merged rows, {npages} pages of <= {br} rows",
        "rows": int(out_rows), "pages": int(npages), "block_rows": br,
        "string_bytes": {"tags": totals[0], "random": totals[1]},
        "warmup": args.warmup, "repeats": args.repeats,
        "device": torch.cuda.get_device_name(0),
        "timing": "device events around each host-synchronous leg",
        "pages_match_oracle": True, "legs": {}}
    for name in legs:
        med = statistics.median(ms[name])
        result["legs"][name] = {"ms_median": med, "ms_min": min(ms[name]),
                                "ms_max": max(ms[name])}
    for c, nm in ((0, "tags"), (1, "random")):
        # every repeat ran the leg twice; the timed run is the second
        cm = [s * 1e3 for s in copy_s[c][1::2][args.warmup:]]
        host = result["legs"]["e_host_" + nm]
        host["copy_ms_median"] = statistics.median(cm)
        host["copy_ms_min"], host["copy_ms_max"] = min(cm), max(cm)
        host["encode_ms_median"] = host["ms_median"] - host["copy_ms_median"]
        dev = result["legs"]["e_dev_" + nm]
        dev["bytes_per_s"] = totals[c] / (dev["ms_median"] / 1e3)
        dev["strings_per_s"] = int(out_rows) / (dev["ms_median"] / 1e3)
    m = {n: result["legs"][n]["ms_median"] for n in legs}
    result["ratios"] = {
        "m_group0_over_m_fields": m["m_group0"] / m["m_fields"],
        "m_group1_minus_group0_ms": m["m_group1"] - m["m_group0"],
        "m_group2_minus_group0_ms": m["m_group2"] - m["m_group0"],
        "e_host_over_e_dev_tags": m["e_host_tags"] / m["e_dev_tags"],
        "e_host_over_e_dev_random": m["e_host_random"] / m["e_dev_random"],
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
