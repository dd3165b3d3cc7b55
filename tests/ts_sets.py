"""Builders of the timestamp-fill tests (test_gpu_ts_tiles.py): sets whose
page sizes sit around every candidate tile of k_rle_ts_tiles, the numpy
expectation of a scan, and a scanner that keeps sentinel-filled output
buffers longer than any result.

Not a test module: nothing here needs a GPU at import."""
import numpy as np

NS = 1_000_000_000
T0 = 1_700_000_000 * NS

# rows per page of one series: 2, 3 and every candidate tile (4096, 8192,
# 16384) -1, +0, +1, then one page of several tiles.  Series s uses the list
# rotated by 4*s, so the same time span meets different tile offsets.
PAGE_ROWS = [2, 3, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385,
             40000]
N_ALL = sum(PAGE_ROWS)  # 126021 rows per series
# first row of page k of series 0
PAGE_FIRST = np.concatenate(([0], np.cumsum(PAGE_ROWS)))

# (delta ns, start offset ns) of the three arange series: 1 s, 10 s (the
# encoder's power-of-ten scaler) and 7 ns (scaler 1; placed in the middle of
# series 0 so a range can cut it)
SERIES = [(NS, 0), (10 * NS, 0), (7, 60_000 * NS)]
# a fourth series of constant-timestamp pages (the encoder emits them as RLE
# with delta 0): (rows, seconds after T0)
CONST_PAGES = [(5, 1000), (4097, 2000), (2, 3000)]

SENTINEL_TS = -0x0123456789ABCDEF
SENTINEL_VAL = -7.25e300


def walk(rng, n):
    return np.round(np.clip(np.cumsum(rng.normal(0, 0.5, n)) + 50, 0, 100), 1)


def page_data(pg, n, dec):
    pg = np.frombuffer(pg, np.uint8)
    hdr = int.from_bytes(pg[0:4].tobytes(), "big")
    return dec(pg[16 + hdr:].tobytes(), n)


def is_rle_time_page(pg):
    """[enc][sub|log10 scale]...: sub 2 is the run-length form."""
    pg = np.frombuffer(pg, np.uint8)
    hdr = int.from_bytes(pg[0:4].tobytes(), "big")
    return int(pg[16 + hdr + 1]) >> 4 == 2


def groups_of(series, nf, seed):
    """series: list of (sid, [ts array per page]).  Returns the groups to
    upload and, per series, (ts, [values per field]) as the oracle decodes
    those very pages."""
    import cnosdb_amd as gs
    from oracle import pyoracle as orc

    rng = np.random.default_rng(seed)
    groups, truth = [], []
    for sid, pages_ts in series:
        dts, dvals = [], [[] for _ in range(nf)]
        for ts in pages_ts:
            n = ts.size
            tp = gs.page_of(ts, gs.CT_TIME)
            assert is_rle_time_page(tp)
            pages = [(tp, gs.CT_TIME)]
            dts.append(page_data(tp, n, orc.decode_i64))
            for f in range(nf):
                vp = gs.page_of(walk(rng, n), gs.CT_F64)
                pages.append((vp, gs.CT_F64))
                dvals[f].append(page_data(vp, n, orc.decode_f64))
            groups.append((sid, pages))
        truth.append((np.concatenate(dts),
                      [np.concatenate(v) for v in dvals]))
    return groups, truth


def split(ts, rows):
    out, r0 = [], 0
    for n in rows:
        out.append(ts[r0:r0 + n])
        r0 += n
    return out


def tile_series():
    """The set of the tile tests: three arange series with the page list
    rotated, and the constant-timestamp series if the encoder makes its
    pages RLE."""
    import cnosdb_amd as gs

    series = []
    for s, (delta, start) in enumerate(SERIES):
        k = (4 * s) % len(PAGE_ROWS)
        rows = PAGE_ROWS[k:] + PAGE_ROWS[:k]
        ts = T0 + start + np.arange(N_ALL, dtype=np.int64) * delta
        series.append((s, split(ts, rows)))
    const = [np.full(n, T0 + sec * NS, dtype=np.int64)
             for n, sec in CONST_PAGES]
    if all(is_rle_time_page(gs.page_of(p, gs.CT_TIME)) for p in const):
        series.append((len(SERIES), const))
    return series


def expect(truth, nf, lo, hi):
    """Closed-range filter and compaction in numpy."""
    out_ts, out_val = [], [[] for _ in range(nf)]
    for ts, vals in truth:
        s = np.searchsorted(ts, lo, side="left")
        e = np.searchsorted(ts, hi, side="right")
        out_ts.append(ts[s:e])
        for f in range(nf):
            out_val[f].append(vals[f][s:e])
    return dict(ts=np.concatenate(out_ts),
                val=np.stack([np.concatenate(v) for v in out_val]))


class Scanner:
    """One uploaded set and output buffers `pad` elements longer than the
    set, pre-filled with a sentinel before every scan unless told not to."""

    def __init__(self, eng, groups, nf, pad=4):
        import torch
        self.eng, self.nf, self.pad = eng, nf, pad
        self.gset = eng.upload(groups)
        rows = self.rows = self.gset.rows
        self.d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
        self.d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
        self.d_ots = torch.empty(rows + pad, dtype=torch.int64, device="cuda")
        self.d_oval = torch.empty(nf * rows + pad, dtype=torch.float64,
                                  device="cuda")
        self.refill()

    def free(self):
        self.gset.free()

    def refill(self):
        self.d_ots.fill_(SENTINEL_TS)
        self.d_oval.fill_(SENTINEL_VAL)

    def launch(self, lo, hi, offset=0, refill=True):
        """scan_fields_async into d_ots[offset:]."""
        import torch
        import cnosdb_amd as gs
        if refill:
            self.refill()
            torch.cuda.synchronize()
        gs.scan_fields_async(self.eng, self.gset, list(range(self.nf)),
                             self.d_ts, self.d_val, (lo, hi),
                             self.d_ots[offset:], self.d_oval)

    def wait(self, offset=0):
        res = self.eng.scan_wait(self.gset)
        return self.collect(int(res.out_rows), offset)

    def scan_sync(self, lo, hi, offset=0):
        """Engine.scan (one field), same buffers."""
        import torch
        assert self.nf == 1
        self.refill()
        torch.cuda.synchronize()
        res = self.eng.scan(self.gset, self.d_ts, self.d_val,
                            time_range=(lo, hi),
                            d_out_ts=self.d_ots[offset:],
                            d_out_val=self.d_oval)
        return self.collect(int(res.out_rows), offset)

    def collect(self, n, offset):
        nf, rows = self.nf, self.rows
        ots = self.d_ots.cpu().numpy()
        oval = self.d_oval.cpu().numpy()
        return dict(
            n=n, ts=ots[offset:offset + n],
            ts_before=ots[:offset], ts_after=ots[offset + n:],
            val=np.stack([oval[f * rows:f * rows + n] for f in range(nf)]),
            val_after=oval[(nf - 1) * rows + n:])


def check(got, exp, what, sentinels=True):
    assert got["n"] == exp["ts"].size, what
    assert got["ts"].dtype == np.int64 and exp["ts"].dtype == np.int64
    assert (got["ts"] == exp["ts"]).all(), what
    assert (got["val"].view(np.uint64)
            == exp["val"].view(np.uint64)).all(), what
    if sentinels:
        assert (got["ts_before"] == SENTINEL_TS).all(), what
        assert (got["ts_after"] == SENTINEL_TS).all(), what
        assert (got["val_after"] == SENTINEL_VAL).all(), what
