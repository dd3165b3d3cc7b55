"""Integer/timestamp decode and page re-encode on the device over the
designed corpus (codec_corpus.py): every simple8b selector, every
timestamp scaler, run-of-ones words, 256-word tile carries, pages with
nulls, row counts that disagree with the data, and the re-encoder's
special values, validity shapes and errors.

Every comparison is exact: decoded values against the oracle's decode of
the same bytes (and the source array where the page is well-formed),
encoded pages byte for byte against the oracle encoder's page."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import cnosdb_amd as gs
import codec_corpus as cc
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = cc.T0
GS_ERR_FORMAT, GS_ERR_CAP, GS_ERR_SENTINEL = -3, -5, -6
ORC_ENC = {"ts": orc.encode_ts, "i64": orc.encode_i64}


@pytest.fixture(scope="module")
def engine():
    e = gs.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def blocks():
    """Oracle-encoded data block of every corpus case, encoded once."""
    return {c.name: ORC_ENC[c.kind](c.values)
            for kind in ("ts", "i64") for c in cc.cases(kind)}


def _bits(x):
    return struct.unpack("<d", struct.pack("<Q", x))[0]


def _sentinel_bits():
    """The value the encoders end every f64 block with, read off the tail
    of a one-value block: [enc][sub][first BE64], then '1' '1', 5 bits
    leading zeros, 6 bits width and the XOR's meaningful bits."""
    enc = orc.encode_f64(np.array([1.0]))
    assert enc == gs.encode_f64(np.array([1.0]))
    prev = int.from_bytes(enc[2:10], "big")
    bits = int.from_bytes(enc[10:], "big")
    nbits = 8 * (len(enc) - 10)

    def take(k, pos):
        return (bits >> (nbits - pos - k)) & ((1 << k) - 1)
    assert take(2, 0) == 0b11
    lead, width = take(5, 2), take(6, 7)
    assert 0 < width < 64
    return prev ^ (take(width, 13) << (64 - lead - width))


def _dummy_f64(n):
    return gs.page_of(np.zeros(n), gs.CT_F64), gs.CT_F64


def _time_page(n):
    return gs.page_of(np.arange(n, dtype=np.int64) * 1000, gs.CT_TIME), \
        gs.CT_TIME


def _groups(kind, pages, ctype=None):
    """pages: [(page bytes, rows)].  ts pages go in slot 0 with a dummy
    field, integer pages in slot 1 behind a plain time page."""
    groups = []
    for i, (pg, n) in enumerate(pages):
        if kind == "ts":
            groups.append((i, [(pg, gs.CT_TIME), _dummy_f64(n)]))
        else:
            groups.append((i, [_time_page(n), (pg, ctype or gs.CT_I64)]))
    return groups


def _decode(engine, groups, col, with_valid=False):
    gset = engine.upload(groups)
    out = torch.zeros(gset.rows, dtype=torch.int64, device="cuda")
    dv = torch.full((gset.rows,), 7, dtype=torch.uint8, device="cuda") \
        if with_valid else None
    engine.decode(gset, col, out, dv)
    offs = gset.row_offsets()
    host = out.cpu().numpy()
    hv = dv.cpu().numpy() if with_valid else None
    gset.free()
    return host, hv, offs


# ------------------------------------------------------------ decode

@pytest.mark.parametrize("kind,ctype", [("ts", gs.CT_TIME),
                                        ("i64", gs.CT_I64),
                                        ("i64", gs.CT_U64)])
def test_decode_corpus_all_valid(engine, blocks, kind, ctype):
    """k_s8b_par over every selector and scaler, k_rle_par over every
    scaler, k_seq_i64 on the uncompressed pages; one set per kind."""
    cases = cc.cases(kind)
    pages = [(gs.build_page(blocks[c.name], c.values.size), c.values.size)
             for c in cases]
    host, hv, offs = _decode(engine, _groups(kind, pages, ctype),
                             0 if kind == "ts" else 1, with_valid=True)
    assert (hv == 1).all()
    for i, c in enumerate(cases):
        n = c.values.size
        got = host[offs[i]:offs[i] + n]
        exp = orc.decode_i64(blocks[c.name], n)
        assert (got == exp).all(), c.name
        assert (got == c.values).all(), f"{c.name} (vs source)"


@pytest.mark.parametrize("pattern", ["first_null", "last_null", "byte0_null"])
def test_decode_i64_corpus_with_nulls(engine, blocks, pattern):
    """A page with a null leaves the parallel kernels for k_seq_i64 and
    its pull-style simple8b iterator, run-of-ones arm included."""
    cases = cc.cases("i64")
    pages, valids = [], []
    for c in cases:
        valid = cc.null_patterns(c.values.size)[pattern]
        valids.append(valid)
        pages.append((gs.build_page(blocks[c.name], valid.size,
                                    np.packbits(valid, bitorder="little")),
                      valid.size))
    host, hv, offs = _decode(engine, _groups("i64", pages), 1,
                             with_valid=True)
    for i, c in enumerate(cases):
        valid = valids[i]
        got = host[offs[i]:offs[i] + valid.size]
        gotv = hv[offs[i]:offs[i] + valid.size]
        exp = orc.decode_i64(blocks[c.name], valid.size, valid)
        src = np.zeros(valid.size, dtype=np.int64)
        src[valid] = c.values
        assert (got == exp).all(), c.name
        assert (got == src).all(), f"{c.name} (vs source)"
        assert (gotv == valid.astype(np.uint8)).all(), f"{c.name} validity"


@pytest.mark.parametrize("kind", ["ts", "i64"])
def test_decode_row_count_mismatch(engine, blocks, kind):
    """Declared rows below the data: the decode stops there.  Above: the
    rows past the last value are 0 (the reference's builder skips them).
    The output buffer is as long as the declared rows either way."""
    sel = [(name, nrows) for name, nrows in cc.ROW_MISMATCH
           if cc.case(name).kind == kind]
    assert len(sel) == 4
    pages = [(gs.build_page(blocks[name], nrows), nrows)
             for name, nrows in sel]
    host, _, offs = _decode(engine, _groups(kind, pages),
                            0 if kind == "ts" else 1)
    assert host.size == sum(nrows for _, nrows in sel)
    for i, (name, nrows) in enumerate(sel):
        got = host[offs[i]:offs[i] + nrows]
        exp = orc.decode_i64(blocks[name], nrows)
        assert (got == exp).all(), (name, nrows)


# -------------------------------------------------------------- scan

def _halves(rng, n):
    """A random walk on a grid of 0.5 in [0, 100]: any sum of a few
    thousand such values is exact in f64 whatever its order, so bucket
    sums compare bit for bit."""
    return np.round(np.clip(np.cumsum(rng.normal(0, 1.0, n)) + 50, 0, 100)
                    * 2) / 2


def _gap_series(s, n=700):
    """Regular 1 s (even s) or 10 s (odd s) series with one missed
    stretch: simple8b with selector-0 and selector-1 words (the gap comes
    120 or more deltas after the first 240)."""
    step = NS if s % 2 == 0 else 10 * NS
    packed = [1] * (n - 1)
    packed[365 + 9 * s] = 5
    return cc.ts_from_deltas(T0 + s, packed, step)


def _scan_set(kinds, seed):
    rng = np.random.default_rng(seed)
    groups, truth = [], []
    for s, k in enumerate(kinds):
        if k == "gap":
            ts = _gap_series(s)
        else:
            ts = T0 + s + np.arange(700, dtype=np.int64) * NS
        tp = gs.build_page(orc.encode_ts(ts), ts.size)
        sub = tp[16 + (ts.size + 7) // 8 + 1] >> 4
        assert sub == (cc.SIMPLE8B if k == "gap" else cc.RLE)
        if k == "gap":
            assert {0, 1} <= cc.selectors_of(orc.encode_ts(ts))
        vals = _halves(rng, ts.size)
        groups.append((s, [(tp, gs.CT_TIME),
                           (gs.page_of(vals, gs.CT_F64), gs.CT_F64)]))
        truth.append((ts, vals))
    return groups, truth


BUCKET_NS = 60 * NS
N_BUCKETS = 120  # 7200 s: past the end of the 10 s series
# on the grid inside the first run-of-ones word of every series / off the
# grid and across the gaps
RANGES = [(T0 + 100 * NS, T0 + 300 * NS),
          (T0 + 50 * NS + NS // 2, T0 + 6000 * NS)]
DEAD = [(T0 + 150 * NS, T0 + 200 * NS)]


def _expect_scan(truth, lo, hi, dead):
    ets, evals = [], []
    emx = np.full(N_BUCKETS, -np.inf)
    esm = np.zeros(N_BUCKETS)
    ect = np.zeros(N_BUCKETS, dtype=np.int64)
    for ts, vals in truth:
        s0, c = orc.time_span(ts, lo, hi)
        ets.append(ts[s0:s0 + c])
        evals.append(vals[s0:s0 + c])
        valid = orc.update_nullbits(ts, dead, np.ones(ts.size, bool))
        m, s, k = orc.bucket_agg(ts[s0:s0 + c], vals[s0:s0 + c],
                                 valid[s0:s0 + c], T0, BUCKET_NS, N_BUCKETS)
        emx = np.maximum(emx, m)
        esm += s
        ect += k
    return np.concatenate(ets), np.concatenate(evals), emx, esm, ect


def _run_scan(engine, gset, lo, hi, dead):
    rows = gset.rows
    d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
    d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
    d_ots = torch.zeros(rows, dtype=torch.int64, device="cuda")
    d_oval = torch.zeros(rows, dtype=torch.float64, device="cuda")
    d_max = torch.full((N_BUCKETS,), -np.inf, dtype=torch.float64,
                       device="cuda")
    d_sum = torch.zeros(N_BUCKETS, dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros(N_BUCKETS, dtype=torch.int64, device="cuda")
    res = engine.scan(gset, d_ts, d_val, time_range=(lo, hi),
                      tombstones=dead, d_out_ts=d_ots, d_out_val=d_oval,
                      agg=dict(bucket_ns=BUCKET_NS, t0=T0,
                               n_buckets=N_BUCKETS, d_max=d_max, d_sum=d_sum,
                               d_count=d_cnt))
    n = int(res.out_rows)
    return (n, d_ots[:n].cpu().numpy(), d_oval[:n].cpu().numpy(),
            d_max.cpu().numpy(), d_sum.cpu().numpy(), d_cnt.cpu().numpy())


def _check_scan(got, exp, rows_too, what):
    n, ots, oval, gmx, gsm, gct = got
    ets, evals, emx, esm, ect = exp
    assert n == ets.size, what
    assert (ots == ets).all(), what
    if rows_too:
        assert (oval.view(np.uint64) == evals.view(np.uint64)).all(), what
    assert (gct == ect).all(), what
    assert (gmx[ect > 0] == emx[ect > 0]).all(), what
    assert (gsm[ect > 0] == esm[ect > 0]).all(), what


def test_scan_general_path_over_run_of_ones_pages(engine):
    """The ordinary non-benchmark time page (a regular series with one
    gap) through the general scan: range ends inside a run-of-ones word,
    a tombstone, bucket aggregates."""
    groups, truth = _scan_set(["gap"] * 8, seed=77)
    gset = engine.upload(groups)
    for lo, hi in RANGES:
        for dead in ([], DEAD):
            got = _run_scan(engine, gset, lo, hi, dead)
            _check_scan(got, _expect_scan(truth, lo, hi, dead),
                        rows_too=not dead, what=(lo - T0, hi - T0, dead))
    gset.free()


def test_scan_mixed_rle_and_gap_groups_leave_the_fused_path(engine):
    """RLE time pages and gap (simple8b) time pages in one set: the fused
    scan needs every time page RLE, so the set takes the general path."""
    groups, truth = _scan_set(["rle", "gap"] * 4, seed=78)
    gset = engine.upload(groups)
    for lo, hi in RANGES:
        got = _run_scan(engine, gset, lo, hi, [])
        _check_scan(got, _expect_scan(truth, lo, hi, []), rows_too=True,
                    what=(lo - T0, hi - T0))
    gset.free()


# --------------------------------------------------------- re-encode

def _pages_out(d_out, cap, lens):
    host = d_out.cpu().numpy()
    return [host[p * cap:p * cap + int(lens[p])].tobytes()
            if lens[p] >= 0 else None for p in range(len(lens))]


def _encode(engine, kind, arrays, d_valid=None, cap=None, base=0):
    """One gs_encode_pages_dev launch over the concatenation of arrays,
    one page per array.  base: rows of filler in front of the first page
    (d_valid then covers them too).  A failed launch raises with .pages
    added: the pages as they were left, None where .lens is negative."""
    rows = np.array([a.size for a in arrays], dtype=np.int32)
    row_off = base + np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(
        np.int64)
    col = np.concatenate(arrays) if len(arrays) else np.zeros(0)
    if base:
        col = np.concatenate([np.full(base, 77, dtype=col.dtype), col])
    if col.size == 0:
        col = np.zeros(1, dtype=arrays[0].dtype)
    d_vals = torch.from_numpy(np.ascontiguousarray(col)).cuda()
    if cap is None:
        cap = int(rows.max()) * 12 + 128
    d_out = torch.zeros(len(arrays) * max(cap, 256), dtype=torch.uint8,
                        device="cuda")
    try:
        lens = engine.encode_pages_dev(kind, d_vals, row_off, rows, d_out,
                                       cap, d_valid=d_valid)
    except RuntimeError as e:
        e.pages = _pages_out(d_out, cap, e.lens)
        raise
    return _pages_out(d_out, cap, lens)


@pytest.mark.parametrize("kind", ["ts", "i64"])
def test_encode_corpus_one_launch(engine, blocks, kind):
    """Every corpus case as one page of a single launch (unequal pages):
    byte-exact with the oracle encoder, and the emitted pages decode on
    the device to the source values."""
    cases = cc.cases(kind)
    pages = _encode(engine, 0 if kind == "ts" else 1,
                    [c.values for c in cases])
    for c, pg in zip(cases, pages):
        exp = gs.build_page(blocks[c.name], c.values.size)
        assert pg == exp, c.name
    host, _, offs = _decode(
        engine, _groups(kind, [(pg, c.values.size)
                               for c, pg in zip(cases, pages)]),
        0 if kind == "ts" else 1)
    for i, c in enumerate(cases):
        got = host[offs[i]:offs[i] + c.values.size]
        assert (got == c.values).all(), c.name


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_encode_300_small_pages_two_workgroups(engine, kind):
    """More than 256 pages: the launch spans two workgroups and each
    builds its own CRC table."""
    rng = np.random.default_rng(300 + kind)
    arrays = []
    for p in range(300):
        n = int(rng.integers(1, 6))
        if kind == 0:
            a = np.sort(rng.integers(0, 2**50, n)).astype(np.int64)
        elif kind == 1:
            a = rng.integers(-2**40, 2**40, n).astype(np.int64)
        else:
            a = np.round(rng.normal(50, 10, n), 2)
        arrays.append(a)
    assert max(a.size for a in arrays) == 5
    pages = _encode(engine, kind, arrays)
    enc = (orc.encode_ts, orc.encode_i64, orc.encode_f64)[kind]
    for p, (a, pg) in enumerate(zip(arrays, pages)):
        bl = int.from_bytes(pg[0:4], "big")
        assert int.from_bytes(pg[12:16], "big") == gs.crc32(pg[16 + bl:]), p
        assert pg == gs.build_page(enc(a), a.size), p


def _special_floats():
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden",
                                       "golden_vectors.json")))
    out = []
    for v in gold["float_special_values"]["values"]:
        out.append(_bits(int(v[5:], 16)) if v.startswith("bits:")
                   else float(v))
    return np.array(out, dtype=np.float64)


def _xor_chain(start_bits, xors):
    bits = [start_bits]
    for x in xors:
        bits.append(bits[-1] ^ x)
    assert _sentinel_bits() not in bits
    return np.array(bits, dtype=np.uint64).view(np.float64)


def _f64_value_cases():
    def span(lead, trail):  # an XOR with exactly these zero counts
        return (1 << (63 - lead)) | (1 << trail)
    return {
        # NaN payloads, +-inf, -0.0, denormals
        "special": _special_floats(),
        # opposite signs and a set low bit: 64 meaningful bits, written
        # as a 6-bit 0; every later XOR then reuses that window
        "xor64": _xor_chain(0x3FF0000000000000,
                            [0x8000000000000001, 0x8000000000000001,
                             span(0, 0) | 0x10, span(12, 12), span(0, 0)]),
        # new window / reuse / new (fewer leading) / reuse / new (fewer
        # trailing) / reuse, then a 40-zero lead, which the format's
        # 5-bit field stores as 8, and a reuse of that
        "window_alternates": _xor_chain(
            0x4049000000000000,
            [span(20, 20), span(24, 24), span(10, 30), span(12, 32),
             span(16, 8), span(16, 9), span(40, 4), span(41, 5)]),
        "n1": np.array([3.25]),
        "n2": np.array([3.25, -1e-300]),
    }


def test_encode_f64_values_one_launch(engine):
    cases = _f64_value_cases()
    pages = _encode(engine, 2, list(cases.values()))
    for (name, vals), pg in zip(cases.items(), pages):
        block = orc.encode_f64(vals)
        assert (orc.decode_f64(block, vals.size).view(np.uint64)
                == vals.view(np.uint64)).all(), name
        assert pg == gs.build_page(block, vals.size), name
        assert pg == gs.page_of(vals, gs.CT_F64), f"{name} (host encoder)"


def test_encode_f64_validity_shapes_one_launch(engine):
    """Nulls at the page edges, one valid row, an all-null page (bitset
    and an empty data region) and a page of no rows.  The null rows hold
    the Gorilla sentinel, which must never be looked at."""
    rng = np.random.default_rng(91)
    sentinel = np.array([_sentinel_bits()], dtype=np.uint64).view(
        np.float64)[0]

    def page(n, valid_rows):
        vals = np.round(np.cumsum(rng.normal(0, 1, n)), 3)
        valid = np.zeros(n, dtype=bool)
        valid[valid_rows] = True
        vals[~valid] = sentinel
        return vals, valid

    shapes = {
        "first_null": page(19, slice(1, None)),
        "last_null": page(24, slice(0, 23)),
        "one_valid_mid": page(21, [10]),
        "all_null": page(13, []),
        "no_rows": (np.zeros(0), np.zeros(0, dtype=bool)),
        "all_valid": page(9, slice(None)),
    }
    valid_col = np.concatenate([v for _, v in shapes.values()])
    d_valid = torch.from_numpy(valid_col.astype(np.uint8)).cuda()
    pages = _encode(engine, 2, [a for a, _ in shapes.values()],
                    d_valid=d_valid)
    for (name, (vals, valid)), pg in zip(shapes.items(), pages):
        assert pg == gs.page_of(vals, gs.CT_F64, valid), name
    alln = pages[list(shapes).index("all_null")]
    assert len(alln) == 16 + 2 and alln[16:] == b"\0\0"
    assert len(pages[list(shapes).index("no_rows")]) == 16


def _small_page_ok(engine):
    """The engine still encodes after an error."""
    vals = np.array([1.5, 2.5, 2.5, -4.0])
    assert _encode(engine, 2, [vals]) == [gs.page_of(vals, gs.CT_F64)]


def test_encode_error_cap(engine):
    with pytest.raises(RuntimeError) as ei:
        _encode(engine, 1, [np.arange(10, dtype=np.int64)], cap=16)
    assert ei.value.status == GS_ERR_CAP
    _small_page_ok(engine)


def test_encode_error_i64_null(engine):
    vals = [np.arange(6, dtype=np.int64) ** 2, np.arange(5, dtype=np.int64)]
    valid = np.ones(11, dtype=np.uint8)
    valid[8] = 0
    with pytest.raises(RuntimeError) as ei:
        _encode(engine, 1, vals, d_valid=torch.from_numpy(valid).cuda())
    assert ei.value.status == GS_ERR_FORMAT
    assert "decode" not in str(ei.value)
    assert ei.value.lens[0] > 0 and ei.value.lens[1] < 0
    assert ei.value.pages[0] == gs.page_of(vals[0], gs.CT_I64)
    _small_page_ok(engine)


# Pages around the 256-row step of the prepare kernel, in one launch whose
# first page does not start at row 0.
_STEP_ROWS = (1, 9, 255, 256, 257, 513)
_STEP_BASE = 7


def test_encode_i64_all_ones_validity_takes_dense_route(engine):
    """kind 1 with a validity array of ones: the column goes through the
    dense scratch column and comes out as the all-valid host pages."""
    rng = np.random.default_rng(411)
    arrays = [rng.integers(-2**40, 2**40, n).astype(np.int64)
              for n in _STEP_ROWS]
    valid = np.ones(_STEP_BASE + sum(_STEP_ROWS), dtype=np.uint8)
    pages = _encode(engine, 1, arrays, base=_STEP_BASE,
                    d_valid=torch.from_numpy(valid).cuda())
    for a, pg in zip(arrays, pages):
        assert pg == gs.page_of(a, gs.CT_I64), a.size


def test_encode_f64_nulls_across_the_prepare_step(engine):
    """kind 2 with about 30 % nulls; rows 255 and 256 (the last of one
    256-row step and the first of the next) are null in the 257-row page
    and valid in the 513-row page.  Null slots hold the Gorilla sentinel."""
    rng = np.random.default_rng(412)
    sentinel = np.array([_sentinel_bits()], dtype=np.uint64).view(
        np.float64)[0]
    arrays, valids = [], []
    for n in _STEP_ROWS:
        vals = np.round(np.cumsum(rng.normal(0, 1, n)), 3)
        valid = rng.random(n) > 0.3
        if n == 257:
            valid[255:257] = False
        if n == 513:
            valid[255:257] = True
        vals[~valid] = sentinel
        arrays.append(vals)
        valids.append(valid)
    valid_col = np.concatenate([np.ones(_STEP_BASE, dtype=bool)] + valids)
    assert 0.2 < 1 - valid_col.mean() < 0.4
    pages = _encode(engine, 2, arrays, base=_STEP_BASE,
                    d_valid=torch.from_numpy(valid_col.astype(np.uint8)).cuda())
    for vals, valid, pg in zip(arrays, valids, pages):
        assert pg == gs.page_of(vals, gs.CT_F64, valid), vals.size


def test_encode_error_ts_null(engine):
    """kind 0 with one null row: GS_ERR_FORMAT with the entry's own
    message, that page's length negative, the other page complete."""
    vals = [T0 + np.arange(40, dtype=np.int64) * 1000,
            T0 + np.arange(300, dtype=np.int64) ** 2]
    valid = np.ones(340, dtype=np.uint8)
    valid[40 + 256] = 0
    with pytest.raises(RuntimeError) as ei:
        _encode(engine, 0, vals, d_valid=torch.from_numpy(valid).cuda())
    assert ei.value.status == GS_ERR_FORMAT
    assert "null row in a ts/i64 page" in str(ei.value)
    assert ei.value.lens[0] > 0 and ei.value.lens[1] < 0
    assert ei.value.pages[0] == gs.page_of(vals[0], gs.CT_TIME)
    _small_page_ok(engine)


def test_encode_error_gorilla_sentinel(engine):
    """The sentinel as a non-first value of one page of five: the status
    the header defines for it, that page's length negative, the other
    four pages complete."""
    rng = np.random.default_rng(17)
    arrays = [np.round(rng.normal(0, 5, n), 2) for n in (7, 12, 9, 1, 30)]
    arrays[2].view(np.uint64)[4] = _sentinel_bits()
    rows =np.array([a.size for a in arrays], dtype=np.int32)
    row_off = np.concatenate([[0], np.cumsum(rows)[:-1]]).astype(np.int64)
    cap = int(rows.max()) * 12 + 128
    d_vals = torch.from_numpy(np.concatenate(arrays)).cuda()
    d_out = torch.zeros(5 * cap, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError) as ei:
        engine.encode_pages_dev(2, d_vals, row_off, rows, d_out, cap)
    assert ei.value.status == GS_ERR_SENTINEL
    assert "decode" not in str(ei.value)
    lens = ei.value.lens
    assert lens[2] < 0
    pages = _pages_out(d_out, cap, lens)
    for p in (0, 1, 3, 4):
        assert pages[p] == gs.build_page(orc.encode_f64(arrays[p]),
                                         arrays[p].size), p
    _small_page_ok(engine)
