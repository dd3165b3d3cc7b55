"""GPU re-encode of string pages (gs_encode_str_pages_dev): every page must
be host.str_page_of's page byte for byte, restated here through the oracle
(orc.encode_str + the page layout), with len, null_count and the min/max
rows checked against a Python min/max over the non-null values.

The block encoder the kernel runs is cnosdb_amd/csrc/gs_str_enc.h;
test_str_enc_cpu.py runs the same source, with the device's loads, under
AddressSanitizer and UBSan over the same corpus."""
import numpy as np
import pytest
import torch

import cnosdb_amd as gs
import str_enc_corpus as ec
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

GS_ERR, GS_ERR_FORMAT, GS_ERR_CAP = -1, -3, -5
NONE = 2**64 - 1
POISON = 0xA5


@pytest.fixture(scope="module")
def engine():
    eng = gs.Engine(0)
    yield eng
    eng.close()


def _column(rows, null_fill=0):
    """Arrow varbinary of rows (bytes or None): offsets, bytes, validity.
    A null row owns null_fill bytes of 0xEE that no page may show."""
    parts = [(b"\xEE" * null_fill) if s is None else s for s in rows]
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(s) for s in parts], out=off[1:])
    data = np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy()
    valid = np.array([s is not None for s in rows], dtype=np.uint8)
    return off, data, valid


def _expect_page(rows):
    present = [s for s in rows if s is not None]
    block = orc.encode_str(present) if present else b""
    return ec.page_layout(block, rows, orc.crc32)


def _expect_stats(rows, base):
    vals = [(s, base + r) for r, s in enumerate(rows) if s is not None]
    if not vals:
        return NONE, NONE
    mn = min(vals)[1]                                  # smallest value, row
    top = max(s for s, _ in vals)
    mx = min(r for s, r in vals if s == top)           # largest, smallest row
    return mn, mx


def _worst(rows):
    p = ec.payload_len(rows)
    return 16 + (len(rows) + 7) // 8 + 2 + 32 + p + p // 6


def _encode(engine, rows, row_off, nrows, valid="auto", null_fill=0,
            cap=None):
    """Encodes the pages (row_off[p], nrows[p]) of the column `rows`;
    returns (info, pages as bytes, cap)."""
    off, data, vd = _column(rows, null_fill)
    pages = [rows[o:o + n] for o, n in zip(row_off, nrows)]
    if cap is None:
        cap = max(_worst(p) for p in pages)
    d_off = torch.from_numpy(off).cuda()
    d_bytes = torch.from_numpy(data).cuda()
    d_valid = None
    if valid == "auto":
        d_valid = torch.from_numpy(vd).cuda()
    d_out = torch.full((len(pages) * cap,), POISON, dtype=torch.uint8,
                       device="cuda")
    info = engine.encode_str_pages_dev(d_off, d_bytes, row_off, nrows, d_out,
                                       cap, d_valid)
    out = d_out.cpu().numpy()
    got = [out[p * cap:p * cap + int(info["len"][p])].tobytes()
           for p in range(len(pages))]
    return info, got, cap


def _check(info, got, rows, row_off, nrows):
    for p, (o, n) in enumerate(zip(row_off, nrows)):
        page = rows[o:o + n]
        want = _expect_page(page)
        assert int(info["len"][p]) == len(want), p
        assert got[p] == want, p
        assert int(info["null_count"][p]) == sum(s is None for s in page), p
        mn, mx = _expect_stats(page, o)
        assert (int(info["min"][p]), int(info["max"][p])) == (mn, mx), p


# ---------------------------------------------------------------- the corpus

CASES = ec.corpus()


@pytest.fixture(scope="module")
def corpus_run(engine):
    """Every corpus case as one page of one column, in one call."""
    rows, row_off, nrows = [], [], []
    for c in CASES:
        row_off.append(len(rows))
        nrows.append(len(c.rows))
        rows.extend(c.rows)
    info, got, _ = _encode(engine, rows, row_off, nrows)
    return rows, row_off, nrows, info, got


@pytest.mark.parametrize("i", range(len(CASES)), ids=[c.name for c in CASES])
def test_corpus_case_is_the_oracles_page(corpus_run, i):
    rows, row_off, nrows, info, got = corpus_run
    _check(info[i:i + 1], got[i:i + 1], rows, row_off[i:i + 1],
           nrows[i:i + 1])


# ------------------------------------------------------- validity and shapes

def _tag_rows(n, seed, null_p=0.0):
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 7, 8, 9, 24, 33, 70], n)
    rows = [b"tag_%d=" % rng.integers(0, 40) +
            bytes(rng.integers(0x30, 0x3a, ln, dtype=np.uint8))
            if ln else b"" for ln in lens]
    if null_p:
        rows = [None if rng.random() < null_p else s for s in rows]
    return rows


N = 300
VALIDITY = {
    "first_row_null": lambda r: r != 0,
    "last_row_null": lambda r: r != N - 1,
    "first_bitset_byte_null": lambda r: r >= 8,
    "scattered_30_percent": None,
    "all_null": lambda r: False,
}


@pytest.mark.parametrize("shape", VALIDITY)
def test_validity_shapes(engine, shape):
    base = 3  # the page starts inside a bitset byte of the column
    rows = _tag_rows(base + N, 11, null_p=0.3 if VALIDITY[shape] is None
                     else 0.0)
    if VALIDITY[shape] is not None:
        rows = [s if r < base or VALIDITY[shape](r - base) else None
                for r, s in enumerate(rows)]
    info, got, _ = _encode(engine, rows, [base], [N])
    _check(info, got, rows, [base], [N])
    if shape == "all_null":
        assert int(info["len"][0]) == 16 + (N + 7) // 8
        assert int(info["min"][0]) == NONE and int(info["max"][0]) == NONE


def test_page_sizes_mid_column_and_zero_rows(engine):
    sizes = [1, 63, 64, 65, 255, 256, 257, 0, 5]
    rows = _tag_rows(5 + sum(sizes), 12, null_p=0.2)
    row_off = list(5 + np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    assert any(o % 8 for o in row_off)
    info, got, _ = _encode(engine, rows, row_off, sizes)
    _check(info, got, rows, row_off, sizes)
    z = sizes.index(0)
    assert int(info["len"][z]) == 16 and got[z] == _expect_page([])


def test_d_valid_null_is_all_valid(engine):
    rows = _tag_rows(200, 13)
    info, got, _ = _encode(engine, rows, [0, 77], [77, 123], valid=None)
    _check(info, got, rows, [0, 77], [77, 123])
    assert not info["null_count"].any()


def test_null_rows_with_bytes_of_their_own(engine):
    rows = _tag_rows(150, 14, null_p=0.4)
    assert any(s is None for s in rows)
    info, got, _ = _encode(engine, rows, [0, 50], [50, 100], null_fill=9)
    _check(info, got, rows, [0, 50], [50, 100])


def test_equal_values_report_the_smallest_row(engine):
    rows = [b"m", None, b"a", b"z", b"a", b"z", b"", b"", b"ab"]
    info, got, _ = _encode(engine, rows, [0, 2], [9, 4])
    _check(info, got, rows, [0, 2], [9, 4])
    assert (int(info["min"][0]), int(info["max"][0])) == (6, 3)
    assert (int(info["min"][1]), int(info["max"][1])) == (2, 3)


@pytest.mark.parametrize("cap_blocks", [1, 3])
def test_350_pages_past_the_grid(engine, cap_blocks):
    per = 9
    rows = _tag_rows(350 * per, 15, null_p=0.1)
    row_off = [p * per for p in range(350)]
    with gs.grid_cap(cap_blocks):
        info, got, _ = _encode(engine, rows, row_off, [per] * 350)
        assert gs.grid_rounds() > 1
    _check(info, got, rows, row_off, [per] * 350)


# -------------------------------------------------------------------- errors

def test_cap_one_below_worst_case_writes_nothing(engine):
    rows = _tag_rows(120, 16, null_p=0.1)
    worst = max(_worst(rows[:60]), _worst(rows[60:]))
    off, data, vd = _column(rows)
    d_off = torch.from_numpy(off).cuda()
    d_bytes = torch.from_numpy(data).cuda()
    d_valid = torch.from_numpy(vd).cuda()
    d_out = torch.full((2 * worst,), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError) as ei:
        engine.encode_str_pages_dev(d_off, d_bytes, [0, 60], [60, 60], d_out,
                                    worst - 1, d_valid)
    assert ei.value.status == GS_ERR_CAP
    assert bool((d_out == POISON).all())
    info, got, _ = _encode(engine, rows, [0, 60], [60, 60], cap=worst)
    _check(info, got, rows, [0, 60], [60, 60])


def test_decreasing_offset_is_refused_and_engine_recovers(engine):
    rows = _tag_rows(100, 17)
    off, data, vd = _column(rows)
    bad = off.copy()
    bad[41] = bad[40] - 1
    d_bytes = torch.from_numpy(data).cuda()
    d_out = torch.full((4096 * 2,), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError) as ei:
        engine.encode_str_pages_dev(torch.from_numpy(bad).cuda(), d_bytes,
                                    [0, 50], [50, 50], d_out, 4096)
    assert ei.value.status == GS_ERR_FORMAT
    assert bool((d_out == POISON).all())
    info, got, _ = _encode(engine, rows, [0, 50], [50, 50])
    _check(info, got, rows, [0, 50], [50, 50])


def test_bad_arguments(engine):
    rows = _tag_rows(10, 18)
    off, data, _ = _column(rows)
    d_off = torch.from_numpy(off).cuda()
    d_bytes = torch.from_numpy(data).cuda()
    d_out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for row_off, nrows in (([], []), ([-1], [5]), ([0], [-5])):
        with pytest.raises(RuntimeError) as ei:
            engine.encode_str_pages_dev(d_off, d_bytes, row_off, nrows, d_out,
                                        4096)
        assert ei.value.status == GS_ERR


# ---------------------------------------------------------------- round trip

def test_round_trip_through_decode_str(engine):
    sizes = [100, 1, 64, 135]
    rows = _tag_rows(sum(sizes), 19, null_p=0.25)
    row_off = list(np.concatenate([[0], np.cumsum(sizes)[:-1]]))
    info, got, _ = _encode(engine, rows, row_off, sizes)
    groups = []
    for g, (o, n) in enumerate(zip(row_off, sizes)):
        ts = np.arange(n, dtype=np.int64) * 10**9
        groups.append((g, [(gs.page_of(ts, gs.CT_TIME), gs.CT_TIME),
                           (got[g], gs.CT_STR)]))
    gset = engine.upload(groups)
    try:
        n = gset.rows
        assert n == len(rows)
        off, data, vd = _column([s if s is not None else None for s in rows])
        total = int(off[-1])
        d_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        d_bytes = torch.zeros(total, dtype=torch.uint8, device="cuda")
        d_valid = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        assert engine.decode_str(gset, 1, d_off, d_bytes, d_valid) == total
        assert (d_off.cpu().numpy() == off).all()
        assert d_bytes.cpu().numpy().tobytes() == data[:total].tobytes()
        assert (d_valid.cpu().numpy() == vd).all()
    finally:
        gset.free()
