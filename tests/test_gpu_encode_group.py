"""gs_encode_group_pages_dev: every page of every column of a merged
column group in one call, with nulls, u64, bool and the page statistics.

Expected page bytes come from the host path (page_of = gs_encode_* over the
non-null values + gs_build_page) and the oracle encoders; expected
statistics from a sequential restatement of the reference's loop
(Page::arrow_array_to_page, tsm/page.rs:137-290) written here."""
import struct

import numpy as np
import pytest
import torch

import cnosdb_amd as gs
from oracle import pyoracle as orc
from test_gpu_codec_edges import _sentinel_bits
from test_gpu_compact_fields import (DTYPES, _expect, _expected_bits,
                                     _mk_streams, _torch_dtype, _upload_raw)

pytestmark = pytest.mark.gpu

GS_ERR, GS_ERR_FORMAT, GS_ERR_CAP, GS_ERR_SENTINEL = -1, -3, -5, -6
T0 = 1_700_000_000_000_000_000
NS = 1_000_000_000
POISON = 0xA5
I64_MAX, I64_MIN, U64_MAX = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1
DBL_MAX = float(np.finfo(np.float64).max)
EDGE_ROWS = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513]
NP_DTYPE = {gs.CT_TIME: np.int64, gs.CT_I64: np.int64, gs.CT_U64: np.uint64,
            gs.CT_F64: np.float64, gs.CT_BOOL: np.uint8}
ORC_ENC = {gs.CT_TIME: orc.encode_ts, gs.CT_I64: orc.encode_i64,
           gs.CT_U64: lambda v: orc.encode_i64(v.view(np.int64)),
           gs.CT_F64: orc.encode_f64, gs.CT_BOOL: orc.encode_bool}


@pytest.fixture(scope="module")
def engine():
    e = gs.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sentinel():
    return np.array([_sentinel_bits()], dtype=np.uint64).view(np.float64)[0]


# ------------------------------------------------------------- harness

def _cap(ctype, maxr):
    """The worst-case page sizes the header gives."""
    bl = (maxr + 7) // 8
    if ctype == gs.CT_F64:
        return 16 + bl + 2 + 8 + (maxr + 1) * 10 + 16
    if ctype == gs.CT_BOOL:
        return 16 + bl + 2 + 10 + bl
    return 16 + bl + 2 + 8 * maxr + 32


def _to_dev(a, pad=3):
    """Column on the device, a few spare elements behind it so that a
    column of no rows still has a buffer."""
    a = np.concatenate([np.ascontiguousarray(a),
                        np.zeros(pad, dtype=a.dtype)])
    if a.dtype == np.uint64:
        a = a.view(np.int64)  # u64 travels as int64 bits
    return torch.from_numpy(a).cuda()


class _Run:
    """One gs_encode_group_pages_dev launch over back-to-back pages.
    cols = [(ctype, values, valid_bool_or_None)], full columns."""

    def __init__(self, engine, cols, page_rows, caps=None, ctypes_override=None):
        self.cols = cols
        self.rows = np.asarray(page_rows, dtype=np.int32)
        self.row_off = np.concatenate(
            [[0], np.cumsum(self.rows)[:-1]]).astype(np.int64)
        self.npages = self.rows.size
        maxr = int(self.rows.max())
        self.caps = caps or [_cap(ct, maxr) for ct, _, _ in cols]
        dcols, self.d_outs = [], []
        for c, (ct, vals, valid) in enumerate(cols):
            assert vals.size == int(self.rows.sum())
            d_vd = None if valid is None else _to_dev(valid.astype(np.uint8))
            if ctypes_override:
                ct = ctypes_override[c]
            dcols.append((ct, _to_dev(vals), d_vd))
            self.d_outs.append(torch.full(
                (self.npages * max(self.caps[c], 1),), POISON,
                dtype=torch.uint8, device="cuda"))
        self.status, self.error = 0, None
        try:
            self.info = engine.encode_group_pages_dev(
                dcols, self.row_off, self.rows,
                list(zip(self.d_outs, self.caps)))
        except RuntimeError as e:
            self.status, self.info, self.error = e.status, e.info, e
        self.host = [d.cpu().numpy() for d in self.d_outs]

    def page(self, c, p):
        n = int(self.info[c]["len"][p])
        assert 16 <= n <= self.caps[c], (c, p, n)
        return self.host[c][p * self.caps[c]:p * self.caps[c] + n].tobytes()

    def src(self, c, p):
        """(values, valid_or_None) of page p of column c."""
        _, vals, valid = self.cols[c]
        lo, hi = int(self.row_off[p]), int(self.row_off[p] + self.rows[p])
        return vals[lo:hi], None if valid is None else valid[lo:hi]

    def expected_page(self, c, p):
        vals, valid = self.src(c, p)
        return gs.page_of(vals, self.cols[c][0], valid)

    def check_pages(self, skip=()):
        for c in range(len(self.cols)):
            for p in range(self.npages):
                if (c, p) in skip:
                    continue
                assert self.page(c, p) == self.expected_page(c, p), \
                    f"column {c} page {p} ({self.rows[p]} rows)"


def _bits_of(ctype, x):
    if ctype == gs.CT_F64:
        return struct.unpack("<Q", struct.pack("<d", x))[0]
    return x & U64_MAX


def _seq_stats(ctype, vals, valid):
    """The reference's loop: sequential over the non-null values, strict
    compares.  Returns (null_count, min bits, max bits)."""
    present = vals if valid is None else vals[valid]
    nulls = vals.size - present.size
    if ctype == gs.CT_BOOL:
        return nulls, 0, 0
    if ctype == gs.CT_F64:
        mn, mx = DBL_MAX, -DBL_MAX
        seq = [float(v) for v in present]
    else:
        mn, mx = (U64_MAX, 0) if ctype == gs.CT_U64 else (I64_MAX, I64_MIN)
        seq = [int(v) for v in present]
    for v in seq:
        if v > mx:
            mx = v
        if v < mn:
            mn = v
    return nulls, _bits_of(ctype, mn), _bits_of(ctype, mx)


def _check_stats(run, skip=()):
    for c, (ct, _, _) in enumerate(run.cols):
        got_min = np.ascontiguousarray(run.info[c]["min"]).view(np.uint64)
        got_max = np.ascontiguousarray(run.info[c]["max"]).view(np.uint64)
        for p in range(run.npages):
            if (c, p) in skip:
                continue
            nulls, mn, mx = _seq_stats(ct, *run.src(c, p))
            what = f"column {c} page {p}"
            assert int(run.info[c]["null_count"][p]) == nulls, what
            assert int(got_min[p]) == mn, f"{what} min {int(got_min[p]):#x}"
            assert int(got_max[p]) == mx, f"{what} max {int(got_max[p]):#x}"


def _gen(rng, ctype, n, sentinel):
    """(values, garbage for null slots)."""
    if ctype == gs.CT_TIME:
        return T0 + np.cumsum(rng.integers(1, 50, n)).astype(np.int64) * NS, None
    if ctype == gs.CT_I64:
        return (np.cumsum(rng.integers(-500, 500, n)).astype(np.int64),
                rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64))
    if ctype == gs.CT_U64:
        v = np.uint64(1 << 63) + np.cumsum(
            rng.integers(-300, 300, n)).astype(np.int64).astype(np.uint64)
        return v, rng.integers(0, U64_MAX, n, dtype=np.uint64)
    if ctype == gs.CT_F64:
        return (np.round(np.cumsum(rng.normal(0, 1, n)) + 50, 2),
                np.full(n, sentinel))
    return rng.integers(0, 2, n, dtype=np.uint8), np.full(n, 0x5A, np.uint8)


def _five_columns(rng, n, sentinel, null_rate=0.3):
    cols = []
    for ct in (gs.CT_TIME, gs.CT_I64, gs.CT_U64, gs.CT_F64, gs.CT_BOOL):
        vals, garbage = _gen(rng, ct, n, sentinel)
        valid = None
        if ct != gs.CT_TIME:
            valid = rng.random(n) >= null_rate
            vals = np.where(valid, vals, garbage).astype(NP_DTYPE[ct])
        cols.append((ct, vals, valid))
    return cols


def _good_call(engine):
    """The engine still encodes after an error."""
    vals = np.array([5, 7, -1, 9, 11], dtype=np.int64)
    valid = np.array([1, 1, 0, 1, 1], dtype=bool)
    run = _Run(engine, [(gs.CT_I64, vals, valid)], [5])
    assert run.status == 0
    run.check_pages()


# -------------------------------------------------- byte-exact per type

@pytest.fixture(scope="module")
def edge_run(engine, sentinel):
    """One launch: the five types over pages at the bitset-byte, wave and
    block edges, laid back to back (odd, unaligned row offsets), ~30 %
    nulls whose value slots hold garbage (the sentinel for f64)."""
    rng = np.random.default_rng(20)
    run = _Run(engine, _five_columns(rng, sum(EDGE_ROWS), sentinel),
               EDGE_ROWS)
    assert run.status == 0, run.error
    return run


@pytest.mark.parametrize("c,name", list(enumerate(["time", "i64", "u64",
                                                   "f64", "bool"])))
def test_byte_exact_per_type(edge_run, c, name):
    ct = edge_run.cols[c][0]
    assert (edge_run.row_off % 8 != 0).any()
    for p, n in enumerate(EDGE_ROWS):
        got = edge_run.page(c, p)
        assert got == edge_run.expected_page(c, p), f"{name} page of {n} rows"
        vals, valid = edge_run.src(c, p)
        present = vals if valid is None else vals[valid]
        bl = (n + 7) // 8
        data = ORC_ENC[ct](present) if present.size else b""
        assert got[16 + bl:] == data, f"{name} page of {n} rows (oracle)"
        if present.size == 0 and ct != gs.CT_F64:
            assert len(got) == 16 + bl


def test_edge_run_statistics(edge_run):
    _check_stats(edge_run)


def test_round_trip_on_device(engine, edge_run):
    """The emitted pages, uploaded as column groups (time, i64, u64, f64,
    bool), decode on the device to the source: values where valid, 0 where
    null, and the validity bytes.  A column group always has rows, so the
    page of no rows stays out."""
    pages = [p for p, n in enumerate(EDGE_ROWS) if n > 0]
    groups = [(i, [(edge_run.page(c, p), edge_run.cols[c][0])
                   for c in range(5)]) for i, p in enumerate(pages)]
    gset = engine.upload(groups)
    offs = gset.row_offsets()
    for c, (ct, _, _) in enumerate(edge_run.cols):
        dt = torch.uint8 if ct == gs.CT_BOOL else \
            torch.float64 if ct == gs.CT_F64 else torch.int64
        d_out = torch.full((gset.rows,), 3, dtype=dt, device="cuda")
        d_vd = torch.full((gset.rows,), 7, dtype=torch.uint8, device="cuda")
        engine.decode(gset, c, d_out, d_vd)
        out = d_out.cpu().numpy()
        out = out if ct == gs.CT_BOOL else out.view(np.uint64)
        vd = d_vd.cpu().numpy()
        for i, p in enumerate(pages):
            vals, valid = edge_run.src(c, p)
            if valid is None:
                valid = np.ones(vals.size, dtype=bool)
            exp = np.where(valid, vals, 0).astype(NP_DTYPE[ct])
            exp = exp if ct == gs.CT_BOOL else exp.view(np.uint64)
            lo = int(offs[i])
            what = f"column {c} page of {vals.size} rows"
            assert vd[lo:lo + vals.size].tolist() == \
                valid.astype(np.uint8).tolist(), what
            assert out[lo:lo + vals.size].tolist() == exp.tolist(), what
    gset.free()


# ------------------------------------------------------ validity shapes

def test_validity_shapes_i64_bool(engine):
    """Nulls at the page edges, one valid row, an all-null page, a page of
    no rows, and exactly 2 and 3 non-null equal-step values (the i64 RLE
    rule needs n > 2) — for a null-carrying i64 and bool column, beside
    all-valid ones passed with d_valid=None in the same call."""
    n = 70
    shapes = {
        "first_null": (n, slice(1, None)),
        "last_null": (n, slice(0, n - 1)),
        "one_valid_mid": (n, [n // 2]),
        "all_null": (n, []),
        "no_rows": (0, []),
        "two_equal_step": (n, [3, 40]),
        "three_equal_step": (n, [3, 40, 69]),
        "byte_edges_null": (n, [i for i in range(n) if i % 8 not in (0, 7)]),
        "all_valid": (n, slice(None)),
    }
    rng = np.random.default_rng(31)
    valid, i64v, boolv, page_rows = [], [], [], []
    for name, (rows, sel) in shapes.items():
        v = np.zeros(rows, dtype=bool)
        v[sel] = True
        k = int(v.sum())
        iv = rng.integers(I64_MIN, I64_MAX, rows, dtype=np.int64)  # garbage
        iv[v] = 1000 + 7 * np.arange(k)  # equal steps over the non-null rows
        bv = np.full(rows, 0x5A, dtype=np.uint8)
        bv[v] = rng.integers(0, 2, k, dtype=np.uint8)
        valid.append(v)
        i64v.append(iv)
        boolv.append(bv)
        page_rows.append(rows)
    valid = np.concatenate(valid)
    total = valid.size
    cols = [
        (gs.CT_I64, np.concatenate(i64v), valid),
        (gs.CT_BOOL, np.concatenate(boolv), valid),
        (gs.CT_I64, np.cumsum(rng.integers(-9, 9, total)).astype(np.int64), None),
        (gs.CT_BOOL, rng.integers(0, 2, total, dtype=np.uint8), None),
    ]
    run = _Run(engine, cols, page_rows)
    assert run.status == 0, run.error
    run.check_pages()
    _check_stats(run)
    names = list(shapes)
    for c in (0, 1):
        assert len(run.page(c, names.index("all_null"))) == 16 + 9
        assert len(run.page(c, names.index("no_rows"))) == 16
    # the RLE rule: 3 equal-step values are run-length coded, 2 are not
    enc = {nm: run.page(0, names.index(nm))[16 + 9 + 1] >> 4
           for nm in ("two_equal_step", "three_equal_step")}
    assert enc == {"two_equal_step": 1, "three_equal_step": 2}


# ----------------------------------------------------------- statistics

def test_statistics_special_values(engine, sentinel):
    """Signed zeros, NaN, infinities, integer extremes, and extrema that
    sit in null slots.  Pages of 4 rows; N marks a null row whose slot
    holds the value written next to it."""
    nan, inf = float("nan"), float("inf")
    S = sentinel

    def N(x):
        return ("null", x)

    f64_pages = [
        [-0.0, 0.0, N(S), N(S)],
        [0.0, -0.0, N(S), N(S)],
        [nan, 1.0, -2.0, N(S)],
        [nan, nan, N(S), N(S)],
        [inf, -inf, 3.0, N(S)],
        [inf, inf, N(-inf), N(S)],
        [1.0, N(-1e300), 2.0, N(1e300)],
        [5.0, -0.0, 0.0, -0.0],
        [-5.0, 0.0, -0.0, N(-0.0)],
        [N(S), N(S), N(S), N(S)],
        [N(-0.0), 0.0, -0.0, nan],
        [DBL_MAX, -DBL_MAX, N(S), N(S)],
    ]
    i64_pages = [
        [I64_MIN, I64_MAX, 0, -1],
        [N(I64_MIN), 5, N(I64_MAX), 6],
        [I64_MAX, N(0), N(0), N(0)],
        [I64_MIN, N(0), N(0), N(0)],
        [N(1), N(2), N(3), N(4)],
        [-1, -1, -1, N(-2)],
    ]
    u64_pages = [
        [(1 << 63) - 1, 1 << 63, 0, U64_MAX],
        [1 << 63, (1 << 63) + 1, N(0), N(U64_MAX)],
        [(1 << 63) - 1, (1 << 63) - 2, N(1 << 63), 7],
        [N(0), N(1), N(2), N(3)],
        [U64_MAX, N(0), N(0), N(0)],
        [0, N(U64_MAX), N(5), N(5)],
    ]
    npages = len(f64_pages)

    def column(ct, pages):
        pages = [pages[p % len(pages)] for p in range(npages)]
        vals, valid = [], []
        for pg in pages:
            for x in pg:
                null = isinstance(x, tuple)
                vals.append(x[1] if null else x)
                valid.append(not null)
        return ct, np.array(vals, dtype=NP_DTYPE[ct]), np.array(valid)

    cols = [column(gs.CT_F64, f64_pages), column(gs.CT_I64, i64_pages),
            column(gs.CT_U64, u64_pages)]
    run = _Run(engine, cols, [4] * npages)
    assert run.status == 0, run.error
    _check_stats(run)
    run.check_pages()
    # spot checks against the issue's wording, independent of _seq_stats
    f = run.info[0]
    zeros = np.ascontiguousarray(f["min"][:2]).view(np.uint64).tolist()
    assert zeros == [1 << 63, 0]  # [-0.0, 0.0] keeps -0.0; [0.0, -0.0] +0.0
    assert f["min"][3] == DBL_MAX and f["max"][3] == -DBL_MAX  # NaN only
    assert f["null_count"][9] == 4 and f["min"][9] == DBL_MAX
    assert f["min"][6] == 1.0 and f["max"][6] == 2.0  # extrema in null slots
    assert run.info[1]["min"][4] == I64_MAX and run.info[1]["max"][4] == I64_MIN
    assert run.info[2]["min"][3] == U64_MAX and run.info[2]["max"][3] == 0


def test_statistics_zero_ties_across_waves(engine, sentinel):
    """The sign of a zero extremum is the first zero's in row order, also
    when the zeros sit in different waves and different 256-row steps of
    the block, and a zero in a null slot does not count."""
    n = 600
    mins = np.full(n, 1.0)
    mins[40], mins[100], mins[300], mins[570] = -0.0, 0.0, -0.0, -0.0
    maxs = np.full(n, -1.0)
    maxs[10], maxs[70], maxs[260], maxs[599] = 0.0, -0.0, 0.0, 0.0
    valid = np.ones(2 * n, dtype=bool)
    valid[40] = False
    valid[n + 10] = False
    valid[[5, 333, n + 200]] = False
    vals = np.concatenate([mins, maxs])
    all_valid = np.concatenate([mins[::-1], maxs[::-1]])
    run = _Run(engine, [(gs.CT_F64, vals, valid),
                        (gs.CT_F64, all_valid, None)], [n, n])
    assert run.status == 0, run.error
    _check_stats(run)
    run.check_pages()
    got = np.ascontiguousarray(run.info[0]["min"]).view(np.uint64)
    assert int(got[0]) == 0  # +0.0 at row 100 precedes -0.0 at row 300
    got = np.ascontiguousarray(run.info[0]["max"]).view(np.uint64)
    assert int(got[1]) == 1 << 63  # -0.0 at row 70 precedes +0.0 at row 260


# ------------------------------------------------- more than 256 blocks

def test_350_work_items(engine, sentinel):
    """5 columns x 70 small pages: more work items than one 256-thread
    workgroup of the page encoder holds; every page byte-exact, its CRC
    field the CRC of its data region."""
    rng = np.random.default_rng(350)
    page_rows = rng.integers(1, 41, 70).tolist()
    run = _Run(engine, _five_columns(rng, sum(page_rows), sentinel),
               page_rows)
    assert run.status == 0, run.error
    run.check_pages()
    _check_stats(run)
    for c in range(5):
        for p, n in enumerate(page_rows):
            pg = run.page(c, p)
            bl = (n + 7) // 8
            assert int.from_bytes(pg[0:4], "big") == bl
            assert int.from_bytes(pg[12:16], "big") == gs.crc32(pg[16 + bl:])


# ----------------------------------------------------------- end to end

def test_merge_then_encode_end_to_end(engine):
    """compact_merge_fields over 3 streams of ~1,200 rows with (f64, i64,
    u64, bool) columns, nulls, and one column absent from the oldest
    stream; its device outputs go, as they are, into one
    encode_group_pages_dev call split at 500-row blocks.  The oracle's
    decode of the new pages is the expected merge, and the folded page
    statistics prune like numpy min/max of the merged data."""
    rng = np.random.default_rng(1200)
    nseries, block_rows = 2, 500
    streams = _mk_streams(rng, [1200, 1190, 1210], nseries, DTYPES,
                          [0.2, 0.1, 0.3, 0.25], absent={(0, 2)})
    gsets, tss, cols = [], [], []
    for per in streams:
        g, t, cs = _upload_raw(engine, per, DTYPES)
        gsets.append(g)
        tss.append(t)
        cols.append(cs)
    total = sum(g.rows for g in gsets)
    d_ots = torch.zeros(total, dtype=torch.int64, device="cuda")
    outs = [(torch.zeros(total, dtype=_torch_dtype(dt), device="cuda"),
             torch.zeros(total, dtype=torch.uint8, device="cuda"))
            for dt in DTYPES]
    out_rows, offs = engine.compact_merge_fields(gsets, tss, cols, d_ots, outs)

    row_off, rows, page_series = [], [], []
    for s in range(nseries):
        r = int(offs[s])
        while r < offs[s + 1]:
            n = min(block_rows, int(offs[s + 1]) - r)
            row_off.append(r)
            rows.append(n)
            page_series.append(s)
            r += n
    npages = len(rows)
    ctypes_ = [gs.CT_TIME, gs.CT_F64, gs.CT_I64, gs.CT_U64, gs.CT_BOOL]
    enc_cols = [(gs.CT_TIME, d_ots, None)] + \
        [(ct, v, vd) for ct, (v, vd) in zip(ctypes_[1:], outs)]
    caps = [_cap(ct, block_rows) for ct in ctypes_]
    d_pages = [torch.zeros(npages * cap, dtype=torch.uint8, device="cuda")
               for cap in caps]
    info = engine.encode_group_pages_dev(enc_cols, row_off, rows,
                                         list(zip(d_pages, caps)))
    host = [d.cpu().numpy() for d in d_pages]

    def page(c, p):
        return host[c][p * caps[c]:p * caps[c] + int(info[c]["len"][p])].tobytes()

    decoders = {gs.CT_F64: orc.decode_f64, gs.CT_I64: orc.decode_i64,
                gs.CT_U64: orc.decode_i64, gs.CT_BOOL: orc.decode_bool}
    stats_exp, stats_got = [], []
    for s in range(nseries):
        mine = [p for p in range(npages) if page_series[p] == s]
        for c, dt in enumerate(DTYPES):
            ct = ctypes_[1 + c]
            uts, sf, sj, valid = _expect(streams, s, c)
            exp = _expected_bits(streams, s, c, dt, sf, sj, valid)
            got_ts, got, got_valid = [], [], []
            for p in mine:
                pt, pv = page(0, p), page(1 + c, p)
                n = int.from_bytes(pv[4:12], "big")
                assert n == rows[p] == int.from_bytes(pt[4:12], "big")
                bl = (n + 7) // 8
                assert int.from_bytes(pt[0:4], "big") == bl
                got_ts.append(orc.decode_i64(pt[16 + bl:], n))
                vd = np.unpackbits(np.frombuffer(pv[16:16 + bl], np.uint8),
                                   bitorder="little")[:n].astype(bool)
                got_valid.append(vd)
                dec = decoders[ct](pv[16 + bl:], n, vd)
                got.append(dec if dt == "bool" else dec.view(np.uint64))
            assert (np.concatenate(got_ts) == uts).all(), f"series {s} ts"
            assert (np.concatenate(got_valid) == valid).all(), (s, dt)
            # null cells are expected as zero
            assert np.concatenate(got).tolist() == exp.tolist(), (s, dt)
        # pruning: folded statistics vs numpy over the expected merge
        uts, sf, sj, valid = _expect(streams, s, 0)
        expv = _expected_bits(streams, s, 0, "f64", sf, sj, valid).view(
            np.float64)
        stats_got += gs.fold_page_stats(info[0][mine[0]:mine[-1] + 1],
                                        info[1][mine[0]:mine[-1] + 1])
        lo = 0
        for p in mine:
            t, v = uts[lo:lo + rows[p]], expv[lo:lo + rows[p]]
            v = v[valid[lo:lo + rows[p]]]
            assert int(info[1]["null_count"][p]) == rows[p] - v.size
            stats_exp.append((int(t.min()), int(t.max()), float(v.min()),
                              float(v.max())))
            lo += rows[p]
    assert int(offs[nseries]) == out_rows == sum(rows)
    assert stats_got == stats_exp
    time_range = (int(T0 + 5000 * NS), int(T0 + 9000 * NS))
    thr = sorted(st[3] for st in stats_exp)[len(stats_exp) // 2 - 1]
    for kw in ({"time_range": time_range}, {"value_pred": ("gt", thr)}):
        keep = gs.prune_column_groups(stats_got, **kw)
        assert keep == gs.prune_column_groups(stats_exp, **kw)
        assert any(keep) and not all(keep), kw
    for g in gsets:
        g.free()


# --------------------------------------------------------------- errors

def test_error_cap_too_small(engine, sentinel):
    rng = np.random.default_rng(5)
    cols = _five_columns(rng, 40, sentinel)
    caps = [_cap(ct, 20) for ct, _, _ in cols]
    caps[4] -= 1  # the bool column one byte short of its worst case
    run = _Run(engine, cols, [20, 20], caps=caps)
    assert run.status == GS_ERR_CAP
    assert all((h == POISON).all() for h in run.host)  # outputs untouched
    _good_call(engine)


def test_error_sentinel_in_one_f64_page(engine, sentinel):
    """The sentinel as a non-first non-null value of one f64 page of a
    five-column call: only that cell is negative, all others byte-exact
    with their statistics."""
    rng = np.random.default_rng(6)
    page_rows = [30, 45, 9]
    cols = _five_columns(rng, sum(page_rows), sentinel)
    ct, vals, valid = cols[3]
    valid[30:36] = [False, True, True, False, True, True]
    vals[30] = sentinel            # null slot: never looked at
    vals[34] = sentinel            # third non-null value of page 1
    run = _Run(engine, cols, page_rows)
    assert run.status == GS_ERR_SENTINEL
    neg = [(c, p) for c in range(5) for p in range(3)
           if run.info[c]["len"][p] < 0]
    assert neg == [(3, 1)]
    run.check_pages(skip={(3, 1)})
    _check_stats(run, skip={(3, 1)})
    _good_call(engine)


def test_error_null_in_time_column(engine, sentinel):
    rng = np.random.default_rng(7)
    cols = _five_columns(rng, 50, sentinel)
    valid = np.ones(50, dtype=bool)
    valid[33] = False
    cols[0] = (gs.CT_TIME, cols[0][1], valid)
    run = _Run(engine, cols, [25, 25])
    assert run.status == GS_ERR_FORMAT
    assert "time" in str(run.error)
    neg = [(c, p) for c in range(5) for p in range(2)
           if run.info[c]["len"][p] < 0]
    assert neg == [(0, 1)]
    run.check_pages(skip={(0, 1)})
    _good_call(engine)


def test_error_string_column(engine):
    vals = np.arange(10, dtype=np.int64)
    run = _Run(engine, [(gs.CT_I64, vals, None), (gs.CT_I64, vals, None)],
               [10], ctypes_override=[gs.CT_I64, gs.CT_STR])
    assert run.status == GS_ERR
    assert all((h == POISON).all() for h in run.host)
    _good_call(engine)


@pytest.mark.parametrize("ncols", [0, 34])
def test_error_ncols(engine, ncols):
    vals = np.arange(10, dtype=np.int64)
    run = _Run(engine, [(gs.CT_I64, vals, None)] * ncols, [10])
    assert run.status == GS_ERR
    assert "ncols" in str(run.error)
    _good_call(engine)
