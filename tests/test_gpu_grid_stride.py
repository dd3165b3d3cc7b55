"""Every capped-grid kernel past its grid.

The kernels of gs_engine.cpp are launched on capped grids (2048 or 65535
blocks) and walk the rest of their work in grid-stride loops, which real
data reaches only beyond 10^9 rows.  cnosdb_amd.grid_cap() lowers the cap
(gs_debug_set_grid_cap), so sets of a few thousand pages drive each kernel
through several trips of its loop: parser state, ring cursors, have/done
flags, LDS slots and carries of the second and later trips, and the ragged
last trip where some lanes of a wave have an item and others have none.

Every case runs at caps of 1 block (most trips) and 3 blocks (a stride that
is no power of two and divides none of the item counts), compares with the
oracle or a numpy restatement — never with an uncapped run of the engine —
and asserts that some launch really went round three times or more
(gs_debug_grid_rounds).  Item counts are asserted not to be multiples of
the strides, so the last trip is ragged.

k_agg_partial_rle and k_build_sgroups_out run in-process here: a bucket of
one row is below the fused-aggregate gate (GS_AGG_FUSED_MIN_ROWS), which
sends a fused-capable scan through the separate aggregate pass."""
import contextlib

import numpy as np
import pytest
import torch

import cnosdb_amd as gs
import codec_corpus as cc
import ts_sets
from oracle import pyoracle as orc
from test_gpu_agg_fused import _expect as agg_expect
from test_gpu_agg_fused import _same_sum, _scan as agg_scan

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = 1_700_000_000 * NS
CAPS = [1, 3]
GOR_CHUNK = 2048   # keep in sync with gs_internal.h
NPAGES = 805       # 3*256 + 37: a 256-thread block takes a 4th, ragged trip


@pytest.fixture(scope="module")
def engine():
    e = gs.Engine(0)
    yield e
    e.close()


@contextlib.contextmanager
def capped(cap):
    """Everything inside, uploads included (k_gor_sync runs at upload), is
    launched on at most `cap` blocks; some launch must have gone round at
    least three times."""
    with gs.grid_cap(cap):
        yield
        assert gs.grid_rounds() >= 3, gs.grid_rounds()


def _ragged(items, per_block=1):
    """items is a multiple of neither stride (cap 1 and cap 3); per_block
    = 1 is a block-per-item kernel, where 7 items or more make three trips
    at cap 3."""
    if per_block == 1:
        assert items % 3 != 0 and items >= 7, items
    else:
        assert items % per_block != 0 and items % (3 * per_block) != 0, items


def _data_len(pg, n):
    return len(pg) - 16 - (n + 7) // 8


def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _tile(parts, n):
    return np.concatenate([parts[i % len(parts)] for i in range(n)])


# ------------------------------------------------------------------ pools

def _nan_page(rng, n):
    v = ts_sets.walk(rng, n)
    nan = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    v[7::97] = nan
    v[11::211] = np.inf
    v[13::223] = -np.inf
    return v


def _rep_walk(rng, n):
    """A walk that repeats its last value nine times in ten: about a
    seventh of a plain walk's bytes."""
    v = ts_sets.walk(rng, n)
    rep = rng.random(n) < 0.9
    for i in range(1, n):
        if rep[i]:
            v[i] = v[i - 1]
    return v


def _alternating(n):
    bits = np.where(np.arange(n) % 2 == 0, 0x3FF0000000000001,
                    0xBFF0000000000000).astype(np.uint64)
    return bits.view(np.float64)


_POOL = {}


def gor_pool(last_rows=1):
    """All-valid f64 pages, listed longest encoding first.  Single-chunk (S)
    and multi-chunk (M) pages alternate in that order, so a thread of
    k_gor_sync that strides the length-sorted PC_GOR table by 256 meets
    M, S, M, S: a recording walk, `continue`, a walk, `continue`."""
    if last_rows not in _POOL:
        rng = np.random.default_rng(20251101)
        full = lambda n: rng.uniform(0, 1e3, n)  # ~8 B per value
        _POOL[last_rows] = [
            _alternating(4097),             # M  3 chunks, 64-bit windows
            ts_sets.walk(rng, 4097),        # M  3 chunks
            _nan_page(rng, 2049),           # M  NaN payloads, infinities
            full(2000),                     # S
            full(1900),                     # S
            ts_sets.walk(rng, 2049),        # M  2 chunks, 1 row in the 2nd
            ts_sets.walk(rng, 2048),        # S  exactly one chunk
            ts_sets.walk(rng, 1500),        # S
            _rep_walk(rng, 4097),           # M
            _rep_walk(rng, 2049),           # M
            ts_sets.walk(rng, 200),         # S  longer than const 4097 rows
            np.full(4097, 42.5),            # M  ~1 bit per value
            np.array([3.25, -0.5][:last_rows]),  # S
        ]
    return _POOL[last_rows]


def gor_groups(pool, n, scan_ts=False, extra=None):
    """n groups, group i holding pool page i % len(pool) behind a time page
    of its length; `extra` = (page bytes, rows) of one more group.  Returns
    (groups, oracle decode of every group, data_len and rows per group)."""
    tpages, vpages, exp = {}, [], []
    for v in pool:
        if v.size not in tpages:
            ts = (T0 + np.arange(v.size, dtype=np.int64) * NS) if scan_ts \
                else np.arange(v.size, dtype=np.int64) * 1000
            tpages[v.size] = (gs.page_of(ts, gs.CT_TIME), ts)
        pg = gs.page_of(v, gs.CT_F64)
        vpages.append(pg)
        exp.append(ts_sets.page_data(pg, v.size, orc.decode_f64))
    groups, dlen, rows = [], [], []
    for i in range(n):
        k = i % len(pool)
        m = pool[k].size
        groups.append((i, [(tpages[m][0], gs.CT_TIME),
                           (vpages[k], gs.CT_F64)]))
        dlen.append(_data_len(vpages[k], m))
        rows.append(m)
    if extra is not None:
        pg, m, ts = extra
        groups.append((n, [(gs.page_of(ts, gs.CT_TIME), gs.CT_TIME),
                           (pg, gs.CT_F64)]))
        dlen.append(_data_len(pg, m))
        rows.append(m)
    truth = [(tpages[pool[i % len(pool)].size][1], [exp[i % len(pool)]])
             for i in range(n)]
    return groups, truth, np.array(dlen), np.array(rows)


def sorted_table(dlen, rows):
    """(is multi-chunk, group index) of the PC_GOR table rows: stable sort
    by data_len, longest first (gs_groups_upload)."""
    order = np.argsort(-dlen, kind="stable")
    return rows[order] > GOR_CHUNK, order


def test_pool_interleaves_in_the_sorted_table():
    """No GPU needed for this one, but it guards the GPU cases' premise."""
    pool = gor_pool()
    _, _, dlen, rows = gor_groups(pool, NPAGES)
    multi, _ = sorted_table(dlen, rows)
    hit = 0
    for t in range(256):
        seq = multi[t::256].tolist()
        hit += any(seq[i:i + 3] == [False, True, False]
                   for i in range(len(seq) - 2))
    assert hit >= 30, hit  # most of a wave of the ragged 4th trip
    # the few-hundred-row page outweighs the constant 4097-row page
    assert dlen[10] > dlen[11] and rows[10] == 200 and rows[11] == 4097
    assert 300 < multi.sum() < 600  # both kinds plentiful
    nch = int(((rows + GOR_CHUNK - 1) // GOR_CHUNK).sum())
    _ragged(NPAGES, 256)
    _ragged(nch, 256)


def _decode_f64(engine, gset, pad=5):
    """Sentinel-filled, over-long outputs: (values, validity, pads)."""
    rows = gset.rows
    out = torch.full((rows + pad,), ts_sets.SENTINEL_VAL,
                     dtype=torch.float64, device="cuda")
    dv = torch.full((rows + pad,), 7, dtype=torch.uint8, device="cuda")
    engine.decode(gset, 1, out, dv)
    out, dv = out.cpu().numpy(), dv.cpu().numpy()
    assert (out[rows:] == ts_sets.SENTINEL_VAL).all() and (dv[rows:] == 7).all()
    return out[:rows], dv[:rows]


# ------------------------------------------- 1. plain Gorilla, all-valid

@pytest.mark.parametrize("cap", CAPS)
def test_gorilla_all_valid(engine, cap):
    """k_gor_sync (upload), k_gor_chunks, k_valid_fill."""
    groups, truth, _, _ = gor_groups(gor_pool(), NPAGES)
    with capped(cap):
        gset = engine.upload(groups)
        # the upload's only launch: 805 pages on one 256-thread block
        assert cap != 1 or gs.grid_rounds() == 4
        try:
            got, gv = _decode_f64(engine, gset)
        finally:
            gset.free()
    exp = np.concatenate([v[0] for _, v in truth])
    assert got.size == exp.size
    assert (_u64(got) == _u64(exp)).all()
    assert (gv == 1).all()


# ------------------------------------------- 2. error surface under stride

def _truncated_page():
    """4097 constant rows, the stream cut at about row 2400: inside the
    second chunk.  Shorter than every other multi-chunk page of the pool,
    so it sits behind them in the sorted table."""
    n = 4097
    data = gs.encode_f64(np.full(n, 7.75))
    cut = data[:10 + 300]
    return gs.build_page(cut, n), n


@pytest.mark.parametrize("cap", CAPS)
def test_truncated_page_in_a_later_round(engine, cap):
    pool = gor_pool(last_rows=2)  # two rows: the time page stays RLE
    pg, n = _truncated_page()
    far = T0 + 10**6 * NS + np.arange(n, dtype=np.int64) * NS
    groups, truth, dlen, rows = gor_groups(pool, NPAGES, scan_ts=True,
                                           extra=(pg, n, far))
    multi, order = sorted_table(dlen, rows)
    at = int(np.flatnonzero(order == NPAGES)[0])
    assert dlen[NPAGES] < dlen[:NPAGES][rows[:NPAGES] > GOR_CHUNK].min()
    assert at >= 3 * 256 - 256 and multi[at]  # a third or later trip at cap 1
    lo, hi = T0 + 100 * NS + NS // 2, T0 + 3000 * NS + NS // 3
    with capped(cap):
        gset = engine.upload(groups)
        try:
            out = torch.zeros(gset.rows, dtype=torch.float64, device="cuda")
            with pytest.raises(RuntimeError, match="shorter"):
                engine.decode(gset, 1, out)
        finally:
            gset.free()
        # the same set without that page decodes clean
        gset = engine.upload(groups[:NPAGES])
        try:
            got, _ = _decode_f64(engine, gset)
        finally:
            gset.free()
        exp = np.concatenate([v[0] for _, v in truth])
        assert (_u64(got) == _u64(exp)).all()
        # a fused scan that leaves the page outside its span succeeds
        sc = ts_sets.Scanner(engine, groups, 1)
        try:
            got = sc.scan_sync(lo, hi)
        finally:
            sc.free()
    ts_sets.check(got, ts_sets.expect(truth, 1, lo, hi), f"cap {cap}")
    assert got["n"] > 10**6


# ------------------------------------------------- 3. Gorilla with nulls

def gorn_pool():
    rng = np.random.default_rng(20251102)

    def tenth(v):
        valid = rng.random(v.size) > 0.10
        valid[0] = True
        return v, valid

    n = 4097
    lead = np.zeros(n, dtype=bool)
    lead[2100:] = True
    trail = np.zeros(n, dtype=bool)
    trail[:1200] = rng.random(1200) > 0.05
    trail[0] = True
    one = np.zeros(2049, dtype=bool)
    one[1500] = True
    return [
        tenth(ts_sets.walk(rng, 2049)), tenth(ts_sets.walk(rng, 4097)),
        tenth(ts_sets.walk(rng, 2048)), tenth(rng.uniform(0, 1e3, 300)),
        (ts_sets.walk(rng, n), lead),     # leading nulls, past chunk 1
        (ts_sets.walk(rng, n), trail),    # sentinel read before chunk 2
        (ts_sets.walk(rng, 2049), one),   # all but one null
        tenth(_nan_page(rng, 2049)), tenth(ts_sets.walk(rng, 700)),
        tenth(_alternating(2049)),
    ]


@pytest.mark.parametrize("cap", CAPS)
def test_gorilla_with_nulls(engine, cap):
    """k_gor_sync_null (upload), k_gor_chunks_null, k_valid_expand: the
    kernel whose wrong second-trip tables were found by the benchmark."""
    pool = gorn_pool()
    npages = 810
    _ragged(npages, 256)
    pages, exp, expv = [], [], []
    for v, valid in pool:
        pg = gs.page_of(v, gs.CT_F64, valid)
        assert _data_len(pg, v.size) >= 10  # PC_GORN, not PC_SEQ
        pages.append((pg, gs.page_of(np.arange(v.size, dtype=np.int64) * 1000,
                                     gs.CT_TIME)))
        exp.append(orc.decode_f64(gs.encode_f64(v[valid]), v.size, valid))
        expv.append(valid.astype(np.uint8))
    nch = sum((pool[i % len(pool)][0].size + GOR_CHUNK - 1) // GOR_CHUNK
              for i in range(npages))
    _ragged(nch, 256)
    groups = [(i, [(pages[i % len(pool)][1], gs.CT_TIME),
                   (pages[i % len(pool)][0], gs.CT_F64)])
              for i in range(npages)]
    with capped(cap):
        gset = engine.upload(groups)
        # the upload's only launch: 810 pages on one 256-thread block
        assert cap != 1 or gs.grid_rounds() == 4
        try:
            got, gv = _decode_f64(engine, gset)
        finally:
            gset.free()
    assert (_u64(got) == _u64(_tile(exp, npages))).all()
    assert (gv == _tile(expv, npages)).all()


# ------------------------- 4. integer, bool, raw and sequential classes

def _decode_int(engine, groups, col, dtype=torch.int64, pad=5):
    gset = engine.upload(groups)
    try:
        rows = gset.rows
        out = torch.full((rows + pad,), 0x5A, dtype=dtype, device="cuda")
        dv = torch.full((rows + pad,), 7, dtype=torch.uint8, device="cuda")
        engine.decode(gset, col, out, dv)
    finally:
        gset.free()
    out, dv = out.cpu().numpy(), dv.cpu().numpy()
    assert (out[rows:] == 0x5A).all() and (dv[rows:] == 7).all()
    return out[:rows], dv[:rows]


@pytest.mark.parametrize("cap", CAPS)
def test_timestamp_corpus(engine, cap):
    """k_rle_par (ts), k_s8b_par and k_seq_i64 over the designed corpus,
    repeated 15 times and a part of a 16th, so that no class holds a
    multiple of three pages."""
    cases = cc.cases("ts")
    n = 15 * len(cases) + 27
    dummy, pages, exp = {}, [], []
    for c in cases:
        m = c.values.size
        blk = orc.encode_ts(c.values)
        pages.append(gs.build_page(blk, m))
        exp.append(orc.decode_i64(blk, m))
        assert (exp[-1] == c.values).all()
        dummy.setdefault(m, gs.page_of(np.zeros(m), gs.CT_F64))
    subs = [cases[i % len(cases)].sub for i in range(n)]
    _ragged(subs.count(cc.RLE)), _ragged(subs.count(cc.SIMPLE8B))
    groups = [(i, [(pages[i % len(cases)], gs.CT_TIME),
                   (dummy[cases[i % len(cases)].values.size], gs.CT_F64)])
              for i in range(n)]
    with capped(cap):
        got, gv = _decode_int(engine, groups, 0)
    assert (got == _tile(exp, n)).all()
    assert (gv == 1).all()


@pytest.mark.parametrize("cap", CAPS)
def test_integer_corpus_with_nulls(engine, cap):
    """k_rle_par (i64), k_s8b_par, and k_seq_i64 over more than 805
    null-carrying and uncompressed pages."""
    cases = cc.cases("i64")
    pages, exp, expv, cls = [], [], [], []
    for c in cases:
        blk = orc.encode_i64(c.values)
        n = c.values.size
        pages.append((gs.build_page(blk, n), n))
        exp.append(orc.decode_i64(blk, n))
        expv.append(np.ones(n, dtype=np.uint8))
        cls.append(c.sub)  # all-valid: a class per sub-encoding
        for valid in cc.null_patterns(n).values():
            pages.append((gs.build_page(blk, valid.size,
                                        np.packbits(valid, bitorder="little")),
                          valid.size))
            exp.append(orc.decode_i64(blk, valid.size, valid))
            expv.append(valid.astype(np.uint8))
            cls.append(cc.UNCOMPRESSED)  # nulls: PC_SEQ like uncompressed
    n = 9 * len(pages) + 106  # 9 times and a part of a 10th
    cls = [cls[i % len(pages)] for i in range(n)]
    assert cls.count(cc.UNCOMPRESSED) >= NPAGES
    _ragged(cls.count(cc.UNCOMPRESSED), 256)
    _ragged(cls.count(cc.RLE)), _ragged(cls.count(cc.SIMPLE8B))
    tpages = {m: gs.page_of(np.arange(m, dtype=np.int64) * 1000, gs.CT_TIME)
              for _, m in pages}
    groups = [(i, [(tpages[pages[i % len(pages)][1]], gs.CT_TIME),
                   (pages[i % len(pages)][0], gs.CT_I64)]) for i in range(n)]
    with capped(cap):
        got, gv = _decode_int(engine, groups, 1)
    assert (got == _tile(exp, n)).all()
    assert (gv == _tile(expv, n)).all()


@pytest.mark.parametrize("cap", CAPS)
def test_bool_and_raw_pages(engine, cap):
    """k_bool_par and k_seq_bool (null-carrying bool pages, 900 of them),
    then k_raw_par over 11 pages of raw big-endian integers."""
    rng = np.random.default_rng(20251103)
    pool, exp, expv = [], [], []
    for k, n in enumerate([300, 1, 65, 7, 64, 257, 9, 100, 33, 8, 2]):
        v = rng.integers(0, 2, n).astype(np.uint8)
        valid = None
        if k >= 2:  # 9 of 11 carry nulls
            valid = rng.random(n) > 0.3
            valid[0], valid[n // 2] = False, True
        pool.append((gs.page_of(v, gs.CT_BOOL, valid), n))
        present = v if valid is None else v[valid]
        exp.append(orc.decode_bool(gs.encode_bool(present), n, valid))
        expv.append(np.ones(n, np.uint8) if valid is None
                    else valid.astype(np.uint8))
    n = 1100
    _ragged(900, 256), _ragged(200)
    tpages = {m: gs.page_of(np.arange(m, dtype=np.int64) * 1000, gs.CT_TIME)
              for _, m in pool}
    groups = [(i, [(tpages[pool[i % 11][1]], gs.CT_TIME),
                   (pool[i % 11][0], gs.CT_BOOL)]) for i in range(n)]
    raw, rexp = [], []
    for m in [1, 3, 255, 256, 257, 1000, 64, 65, 513, 2, 700]:
        v = rng.integers(-2**62, 2**62, m).astype(np.int64)
        blk = bytes([1]) + v.astype(">i8").tobytes()  # Encoding::Null
        raw.append((len(raw), [
            (gs.page_of(np.arange(m, dtype=np.int64) * 1000, gs.CT_TIME),
             gs.CT_TIME), (gs.build_page(blk, m), gs.CT_I64)]))
        rexp.append(orc.decode_i64(blk, m))
    _ragged(len(raw))
    with capped(cap):
        got, gv = _decode_int(engine, groups, 1, dtype=torch.uint8)
        gs.grid_rounds(reset=True)
        rgot, rv = _decode_int(engine, raw, 1)
    assert (got == _tile(exp, n)).all()
    assert (gv == _tile(expv, n)).all()
    assert (rgot == np.concatenate(rexp)).all() and (rv == 1).all()


# ------------------------------------------------------------- 5. strings

def str_pool():
    """(page, per-row lengths with 0 for null, payload bytes, validity)."""
    rng = np.random.default_rng(20251104)
    tags = [b"hostname=host_%04d" % i for i in range(16)]
    out = []
    for k, n in enumerate([1, 40, 7, 33, 16, 25, 2, 39, 12, 20, 5, 9, 31]):
        strs = [tags[int(rng.integers(0, 16))] if rng.random() < 0.6 else
                bytes(rng.integers(0, 256, int(rng.integers(0, 50)))
                      .astype(np.uint8)) for _ in range(n)]
        valid = None
        if k % 3 == 1:
            valid = rng.random(n) > 0.25
        present = [s for i, s in enumerate(strs) if valid is None or valid[i]]
        if k % 4 == 3:  # uncompressed block: [1] then [u64 BE len][bytes]...
            blk = bytes([1]) + b"".join(len(s).to_bytes(8, "big") + s
                                        for s in present)
        else:
            blk = gs.encode_str(present)
        bitset = None if valid is None else np.packbits(valid,
                                                        bitorder="little")
        dec = orc.decode_str(blk, n, valid)
        out.append((gs.build_page(blk, n, bitset),
                    np.array([0 if s is None else len(s) for s in dec],
                             dtype=np.int64),
                    np.frombuffer(b"".join(s for s in dec if s is not None),
                                  dtype=np.uint8),
                    np.array([s is not None for s in dec], dtype=np.uint8)))
    return out


@pytest.mark.parametrize("cap", CAPS)
def test_strings(engine, cap):
    """k_str_decode (thread per page), k_scan_add and k_str_gather (thread
    per row) over 819 small snappy and uncompressed pages."""
    pool = str_pool()
    n = 819
    _ragged(n, 256)
    tpages = {p[1].size: gs.page_of(np.arange(p[1].size, dtype=np.int64)
                                    * 1000, gs.CT_TIME) for p in pool}
    groups = [(i, [(tpages[pool[i % 13][1].size], gs.CT_TIME),
                   (pool[i % 13][0], gs.CT_STR)]) for i in range(n)]
    lens = _tile([p[1] for p in pool], n)
    data = _tile([p[2] for p in pool], n)
    valid = _tile([p[3] for p in pool], n)
    _ragged(lens.size, 256)
    with capped(cap):
        gset = engine.upload(groups)
        try:
            rows = gset.rows
            assert rows == lens.size
            d_off = torch.full((rows + 1 + 3,), -5, dtype=torch.int64,
                               device="cuda")
            d_bytes = torch.full((data.size + 16,), 0x5A, dtype=torch.uint8,
                                 device="cuda")
            d_valid = torch.full((rows + 3,), 7, dtype=torch.uint8,
                                 device="cuda")
            total = engine.decode_str(gset, 1, d_off, d_bytes, d_valid)
        finally:
            gset.free()
    off = d_off.cpu().numpy()
    assert total == data.size
    assert (off[:rows + 1] == np.concatenate(([0], np.cumsum(lens)))).all()
    assert (off[rows + 1:] == -5).all()
    got = d_bytes.cpu().numpy()
    assert (got[:total] == data).all() and (got[total:] == 0x5A).all()
    gv = d_valid.cpu().numpy()
    assert (gv[:rows] == valid).all() and (gv[rows:] == 7).all()


# ---------------------------------------------------------- 6. fused scan

SIZES = [2049, 4100, 3001, 2600, 4097, 3500, 2050]
NSERIES, PAGES_PER_SERIES, NVAR = 7, 115, 3


def fused_set():
    """7 series of 115 pages (805 groups, 2049..4100 rows a page, 1 s a
    row), two fields.  The series share their time pages; value pages come
    from a pool of three per size, rotated by series, page and field."""
    if "fused" in _POOL:
        return _POOL["fused"]
    rng = np.random.default_rng(20251105)
    vpool = {m: [gs.page_of(ts_sets.walk(rng, m), gs.CT_F64)
                 for _ in range(NVAR)] for m in SIZES}
    vdec = {m: [ts_sets.page_data(pg, m, orc.decode_f64) for pg in vpool[m]]
            for m in SIZES}
    tpages, tdec, r0 = [], [], 0
    for p in range(PAGES_PER_SERIES):
        m = SIZES[p % len(SIZES)]
        tp = gs.page_of(T0 + (r0 + np.arange(m, dtype=np.int64)) * NS,
                        gs.CT_TIME)
        assert ts_sets.is_rle_time_page(tp)
        tpages.append(tp)
        tdec.append(ts_sets.page_data(tp, m, orc.decode_i64))
        r0 += m
    ts_all = np.concatenate(tdec)
    groups, truth = [], []
    for s in range(NSERIES):
        vals = [[], []]
        for p in range(PAGES_PER_SERIES):
            m = SIZES[p % len(SIZES)]
            k = [(s + p + f) % NVAR for f in range(2)]
            groups.append((s, [(tpages[p], gs.CT_TIME),
                               (vpool[m][k[0]], gs.CT_F64),
                               (vpool[m][k[1]], gs.CT_F64)]))
            for f in range(2):
                vals[f].append(vdec[m][k[f]])
        truth.append((ts_all, [np.concatenate(v) for v in vals]))
    nch = NSERIES * sum((SIZES[p % len(SIZES)] + GOR_CHUNK - 1) // GOR_CHUNK
                        for p in range(PAGES_PER_SERIES))
    _POOL["fused"] = (groups, truth, r0, nch)
    return _POOL["fused"]


def _check_agg(got, truth, nf, q, what):
    ets, evals, emx, esm, ect = agg_expect(truth, nf, *q)
    assert got["ts"].size == ets.size, what
    assert (got["ts"] == ets).all(), what
    for f in range(nf):
        assert (_u64(got["val"][f]) == _u64(evals[f])).all(), what
    assert (got["ct"] == ect).all(), what
    assert (_u64(got["mx"]) == _u64(emx)).all(), what
    _same_sum(got["sm"], esm, what)  # rtol 1e-12, as test_gpu_agg_fused.py
    return ect


@pytest.mark.parametrize("cap", CAPS)
def test_fused_scan(engine, cap):
    """k_spans_rle, k_scan_add, k_rle_ts_tiles, k_gor_active, both
    k_gor_chunks_filtered, k_agg_fixup, k_agg_merge; with one-row buckets
    k_build_sgroups_out and k_agg_partial_rle."""
    groups, truth, nrows, nch = fused_set()
    assert len(groups) == NPAGES and NSERIES * nrows < 3_000_000
    _ragged(len(groups), 256), _ragged(nch, 256), _ragged(NSERIES)
    # the range starts and ends inside a chunk, between two rows, and
    # leaves the chunks of the first 16 and the last 16 pages inactive
    lo = T0 + 50_123 * NS - NS // 2
    hi = T0 + 300_777 * NS + NS // 3
    assert hi < T0 + (nrows - 40_000) * NS
    # 300 s buckets with edges at rows = 37 mod 300: six or more inside a
    # chunk, the first and last shared with the neighbouring chunks; the
    # grid ends before the range does
    nb = 1001
    _ragged((nb + 3) // 4)  # blocks of k_agg_merge
    q300 = (lo, hi, T0 - 263 * NS, 300 * NS, nb)
    # one-row buckets: below the gate, the separate aggregate pass
    nb1 = 8191
    _ragged((nb1 + 3) // 4)
    q1 = (lo, hi, T0 + 50_100 * NS, NS, nb1)
    with capped(cap):
        sc = ts_sets.Scanner(engine, groups, 2)
        try:
            sc.launch(lo, hi)            # two fields, no aggregate
            plain = sc.wait()
            two = agg_scan(engine, sc.gset, 2, *q300)   # scan_fields
            one = agg_scan(engine, sc.gset, 1, *q300)   # engine.scan
            sep = agg_scan(engine, sc.gset, 2, *q1)
        finally:
            sc.free()
    ts_sets.check(plain, ts_sets.expect(truth, 2, lo, hi), f"cap {cap}")
    ect = _check_agg(two, truth, 2, q300, f"cap {cap} two fields")
    assert (ect[0, 168:1001] == NSERIES * 300).all() and ect[0, :167].sum() == 0
    _check_agg(one, [(t, v[:1]) for t, v in truth], 1, q300,
               f"cap {cap} one field")
    ect = _check_agg(sep, truth, 2, q1, f"cap {cap} one-row buckets")
    assert (ect[:, 23:] == NSERIES).all() and ect[:, :23].sum() == 0


# -------------------------------------------------------- 7. general scan

def _agg_bufs(nb):
    return dict(d_max=torch.full((nb,), -np.inf, dtype=torch.float64,
                                 device="cuda"),
                d_sum=torch.zeros(nb, dtype=torch.float64, device="cuda"),
                d_count=torch.zeros(nb, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("cap", CAPS)
def test_general_scan(engine, cap):
    """k_spans, k_tombstone, k_vmask, k_compact_masked, k_compact,
    k_agg_partial over 805 small null-carrying groups, expected as in
    test_scan_fuzz_vs_oracle."""
    rng = np.random.default_rng(20251106)
    sizes = [37, 300, 7, 100, 257, 64, 1]           # one series, 766 rows
    per = sum(sizes)
    vpool = []
    for m in sizes:
        for _ in range(2):
            v = ts_sets.walk(rng, m)
            valid = rng.random(m) > 0.2
            valid[0] = True
            vpool.append((gs.page_of(v, gs.CT_F64, valid), v, valid))
    nseries = 115
    tpages, r0 = [], 0
    for m in sizes:
        tpages.append(gs.page_of(T0 + (r0 + np.arange(m, dtype=np.int64)) * NS,
                                 gs.CT_TIME))
        r0 += m
    ts = T0 + np.arange(per, dtype=np.int64) * NS
    groups, truth = [], []
    for s in range(nseries):
        vs, vd = [], []
        for p, m in enumerate(sizes):
            pg, v, valid = vpool[2 * p + (s + p) % 2]
            groups.append((s, [(tpages[p], gs.CT_TIME), (pg, gs.CT_F64)]))
            vs.append(v), vd.append(valid)
        truth.append((np.concatenate(vs), np.concatenate(vd)))
    assert len(groups) == NPAGES
    _ragged(NPAGES, 256), _ragged(nseries)
    lo, hi = T0 + 20 * NS, T0 + 700 * NS + NS // 2   # cuts pages 0 and 4
    tomb = [(T0 + 330 * NS, T0 + 470 * NS)]          # pages 1..4
    pred = ("gt", 50.0)
    nb, bucket, t0 = 29, 25 * NS, T0 + 5 * NS
    _ragged((nb + 3) // 4)
    res = {}
    with capped(cap):
        gset = engine.upload(groups)
        try:
            rows = gset.rows
            for name, p in (("pred", pred), ("time", None)):
                d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
                d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
                d_ots = torch.full((rows + 4,), ts_sets.SENTINEL_TS,
                                   dtype=torch.int64, device="cuda")
                d_oval = torch.full((rows + 4,), ts_sets.SENTINEL_VAL,
                                    dtype=torch.float64, device="cuda")
                agg = dict(bucket_ns=bucket, t0=t0, n_buckets=nb,
                           **_agg_bufs(nb))
                r = engine.scan(gset, d_ts, d_val, time_range=(lo, hi),
                                tombstones=tomb, d_out_ts=d_ots,
                                d_out_val=d_oval, agg=agg, value_pred=p)
                res[name] = (int(r.out_rows), d_ots.cpu().numpy(),
                             d_oval.cpu().numpy(),
                             {k: agg[k].cpu().numpy()
                              for k in ("d_max", "d_sum", "d_count")})
        finally:
            gset.free()
    m = (ts >= lo) & (ts <= hi)
    tm = (ts >= tomb[0][0]) & (ts <= tomb[0][1])
    for name, p in (("pred", pred), ("time", None)):
        ets, ev = [], []
        emx, esm, ect = np.full(nb, -np.inf), np.zeros(nb), np.zeros(nb, np.int64)
        for vals, valid in truth:
            vmask = valid & ~tm
            if p:   # DataFilter: null and deleted rows fail the predicate
                sel = m & vmask & (vals > p[1])
                v = vals[sel]
                amask = sel
            else:   # time filter: every span row travels, nulls as 0.0
                sel = m
                v = vals[sel].copy()
                v[~valid[sel]] = 0.0
                amask = m & vmask
            ets.append(ts[sel]), ev.append(v)
            mx, sm, ct = orc.bucket_agg(ts, vals, amask, t0, bucket, nb)
            emx, esm, ect = np.maximum(emx, mx), esm + sm, ect + ct
        ets, ev = np.concatenate(ets), np.concatenate(ev)
        n, gts, gval, agg = res[name]
        what = f"cap {cap} {name}"
        assert n == ets.size, what
        assert (gts[:n] == ets).all(), what
        assert (_u64(gval[:n]) == _u64(ev)).all(), what
        assert (gts[n:] == ts_sets.SENTINEL_TS).all(), what
        assert (gval[n:] == ts_sets.SENTINEL_VAL).all(), what
        assert (agg["d_count"] == ect).all(), what
        nz = ect > 0
        assert nz.sum() >= 20
        assert (agg["d_max"][nz] == emx[nz]).all(), what
        _same_sum(agg["d_sum"][nz], esm[nz], what)


# -------------------------------------------------------- 8. group by tag

@pytest.mark.parametrize("cap", CAPS)
def test_group_by_tag(engine, cap):
    """k_tag_series and k_agg_tag over 805 series of one 40-row page and 41
    tags; the one-row buckets also take k_build_sgroups_out and
    k_agg_partial_rle through 805 series groups."""
    rng = np.random.default_rng(20251107)
    nseries, m, ntags, nv = NPAGES, 40, 41, 8
    ts = T0 + np.arange(m, dtype=np.int64) * NS
    tpage = gs.page_of(ts, gs.CT_TIME)
    vals = [ts_sets.walk(rng, m) for _ in range(nv)]
    vpages = [gs.page_of(v, gs.CT_F64) for v in vals]
    vals = [ts_sets.page_data(pg, m, orc.decode_f64) for pg in vpages]
    tags = [b"host_%02d" % t for t in range(ntags)]
    spages = [gs.str_page_of([t] * m) for t in tags]
    groups = [(s, [(tpage, gs.CT_TIME), (vpages[s % nv], gs.CT_F64),
                   (spages[s % ntags], gs.CT_STR)]) for s in range(nseries)]
    lo, hi = T0 + 3 * NS, T0 + 36 * NS
    nb = m
    _ragged(nseries, 256), _ragged(ntags * nb, 256)
    capg = 64
    with capped(cap):
        gset = engine.upload(groups)
        try:
            rows = gset.rows
            d_ts = torch.zeros(rows, dtype=torch.int64, device="cuda")
            d_val = torch.zeros(rows, dtype=torch.float64, device="cuda")
            d_ots = torch.zeros(rows, dtype=torch.int64, device="cuda")
            d_oval = torch.zeros(rows, dtype=torch.float64, device="cuda")
            agg = dict(bucket_ns=NS, t0=T0, n_buckets=nb, **_agg_bufs(nb))
            engine.scan(gset, d_ts, d_val, time_range=(lo, hi),
                        d_out_ts=d_ots, d_out_val=d_oval, agg=agg)
            d_off = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
            d_bytes = torch.zeros(rows * 8, dtype=torch.uint8, device="cuda")
            engine.decode_str(gset, 2, d_off, d_bytes)
            g_max = torch.zeros(capg * nb, dtype=torch.float64, device="cuda")
            g_sum = torch.zeros(capg * nb, dtype=torch.float64, device="cuda")
            g_cnt = torch.zeros(capg * nb, dtype=torch.int64, device="cuda")
            ngids, rep = gs.groupby_tag(engine, gset, nb, g_max, g_sum, g_cnt,
                                        capg)
        finally:
            gset.free()
    assert ngids == ntags
    off, data = d_off.cpu().numpy(), d_bytes.cpu().numpy()
    assert [data[off[r]:off[r + 1]].tobytes() for r in rep] == tags
    gm = g_max.cpu().numpy().reshape(capg, nb)[:ngids]
    gsm = g_sum.cpu().numpy().reshape(capg, nb)[:ngids]
    gc = g_cnt.cpu().numpy().reshape(capg, nb)[:ngids]
    sel = (ts >= lo) & (ts <= hi)
    for t in range(ntags):
        members = [s for s in range(nseries) if s % ntags == t]
        v = np.stack([vals[s % nv] for s in members])   # [series, bucket]
        assert (gc[t] == np.where(sel, len(members), 0)).all(), t
        assert (gm[t][sel] == v.max(axis=0)[sel]).all(), t
        assert np.allclose(gsm[t][sel], v.sum(axis=0)[sel], rtol=1e-12), t
    # the scan's own totals came through k_agg_partial_rle and k_agg_merge
    assert (agg["d_count"].cpu().numpy() == np.where(sel, nseries, 0)).all()


# ---------------------------------------------------------- 9. compaction

@pytest.mark.parametrize("cap", CAPS)
def test_compaction(engine, cap):
    """k_cm_flags, k_cm_prefix, k_cm_scatter_fields, then the same three
    at ncols=1 (gs_compact_merge of column 0): 11 series, 3 streams,
    columns with nulls and one absent column.  k_cm_prefix has 3 x 11 = 33 items, which
    the 3-block stride divides: 11 whole trips at cap 3, 33 at cap 1."""
    import test_gpu_compact_fields as cf
    nseries = 11
    _ragged(nseries)
    r = np.random.default_rng(20251108)
    streams = cf._mk_streams(r, [300, 200, 250], nseries, cf.DTYPES,
                             [0.3, 0.0, 0.2, 0.5], absent={(1, 2)})
    with capped(cap):
        m = cf._merge(engine, streams, cf.DTYPES)
        try:
            rows, offs, gts, gbits, gvd = cf._per_column_merge(engine, m, 0)
        finally:
            cf._free(m)
    cf._check(m, streams, cf.DTYPES, nseries, tag=f"cap {cap}")
    assert rows == m.out_rows and (offs == m.offs).all()
    for s in range(nseries):
        uts, sf, sj, valid = cf._expect(streams, s, 0)
        lo, hi = offs[s], offs[s + 1]
        assert (gts[lo:hi] == uts).all(), s
        assert (gvd[lo:hi] == valid.astype(np.uint8)).all(), s
        exp = cf._expected_bits(streams, s, 0, "f64", sf, sj, valid)
        assert (gbits[lo:hi][valid] == exp[valid]).all(), s


# -------------------------------------------------------- 10. device encode

@pytest.mark.parametrize("cap", CAPS)
def test_encode_pages(engine, cap):
    """gs_encode_pages_dev, the one-column case of the group encode: 1573
    pages of 1..40 rows for each of its three kinds, byte-exact against the
    host encoders.  k_enc_prepare takes a page per block; k_enc_group_pages
    takes a page per thread in 64-thread blocks: 8 * 192 + 37 pages make a
    ragged ninth trip at cap 3, and a ragged 25th at cap 1."""
    rng = np.random.default_rng(20251109)
    npages = 1573
    _ragged(npages)
    _ragged(npages, 64)
    rows = (1 + (np.arange(npages) * 7) % 40).astype(np.int32)
    row_off = np.concatenate(([0], np.cumsum(rows)[:-1])).astype(np.int64)
    total = int(rows.sum())
    page_of_row = np.repeat(np.arange(npages), rows)
    # every third page regular (run-length coded), the others jittered
    jit = np.where(page_of_row % 3 == 0, 0, rng.integers(0, NS // 2, total))
    ts = T0 + np.arange(total, dtype=np.int64) * NS + jit
    i64 = np.where(page_of_row % 4 == 0, 42,
                   np.cumsum(rng.integers(-500, 500, total))).astype(np.int64)
    f64 = ts_sets.walk(rng, total)
    valid = rng.random(total) > 0.3
    valid[row_off] = True  # a value in every page
    cols = [(0, gs.CT_TIME, ts, None), (1, gs.CT_I64, i64, None),
            (2, gs.CT_F64, f64, None), (2, gs.CT_F64, f64, valid)]
    capb = 1024
    got = []
    with capped(cap):
        for kind, _, v, vd in cols:
            d_out = torch.full((npages * capb,), 0xA5, dtype=torch.uint8,
                               device="cuda")
            d_vd = None if vd is None else \
                torch.from_numpy(vd.astype(np.uint8)).cuda()
            lens = engine.encode_pages_dev(kind, torch.from_numpy(v).cuda(),
                                           row_off, rows, d_out, capb,
                                           d_valid=d_vd)
            got.append((lens, d_out.cpu().numpy()))
    for (kind, ct, v, vd), (lens, host) in zip(cols, got):
        for p in range(npages):
            sl = slice(int(row_off[p]), int(row_off[p] + rows[p]))
            exp = gs.page_of(v[sl], ct, None if vd is None else vd[sl])
            assert host[p * capb:p * capb + lens[p]].tobytes() == exp, \
                (kind, vd is not None, p)


@pytest.mark.parametrize("cap", CAPS)
def test_encode_group(engine, cap):
    """k_enc_prepare (block per work item) and k_enc_group_pages (thread
    per work item, 64-thread blocks): 31 columns x 8 pages = 248 items.
    Work items are column-major, so the 64 items of a block span nine
    columns; neighbouring columns differ in type and in whether they carry
    nulls.  Pages byte-exact, statistics as the sequential restatement of
    test_gpu_encode_group.py."""
    import test_gpu_encode_group as eg
    from test_gpu_codec_edges import _sentinel_bits
    sentinel = np.array([_sentinel_bits()], dtype=np.uint64).view(np.float64)[0]
    rng = np.random.default_rng(20251110)
    page_rows = [513, 1, 257, 8, 64, 300, 9, 40]
    n = sum(page_rows)
    kinds = [(gs.CT_I64, True), (gs.CT_F64, False), (gs.CT_BOOL, True),
             (gs.CT_U64, False), (gs.CT_F64, True), (gs.CT_I64, False),
             (gs.CT_U64, True), (gs.CT_BOOL, False)]
    cols = [(gs.CT_TIME, eg._gen(rng, gs.CT_TIME, n, sentinel)[0], None)]
    for c in range(30):
        ct, nulls = kinds[c % len(kinds)]
        vals, garbage = eg._gen(rng, ct, n, sentinel)
        valid = None
        if nulls:
            valid = rng.random(n) >= 0.3
            vals = np.where(valid, vals, garbage).astype(eg.NP_DTYPE[ct])
        cols.append((ct, vals, valid))
    for a, b in zip(cols[1:], cols[2:]):
        assert a[0] != b[0] and (a[2] is None) != (b[2] is None)
    nwork = len(cols) * len(page_rows)
    assert nwork >= 229
    _ragged(nwork, 64), _ragged(nwork)
    with capped(cap):
        run = eg._Run(engine, cols, page_rows)
    assert run.status == 0, run.error
    run.check_pages()
    eg._check_stats(run)
