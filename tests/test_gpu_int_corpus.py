"""GPU decode of integer, timestamp and bool pages through the kernels that
share cnosdb_amd/csrc/gs_int_dec.h (k_rle_par, k_s8b_par, k_bool_par,
k_seq_i64, k_seq_bool, k_spans_rle) over the pages of tests/int_corpus.py:
every corpus page whole and cut short must decode to what the oracle
decodes, every designed malformed page must fail gs_decode with the
message of its verdict, and the fused scan must refuse an RLE time page
that gs_decode refuses.

The header also compiles as host C++.  No malformed page is uploaded
before the host program (tests/cpu/int_decode_check.cpp) has given the
expected verdict on it in this very run; test_int_decode_cpu.py runs the
same program under AddressSanitizer and UBSan."""
import numpy as np
import pytest
import torch

import cnosdb_amd as gs
import codec_corpus as cc
import int_corpus as ic
import ts_sets as S
from oracle import pyoracle as orc

pytestmark = pytest.mark.gpu

GS_ERR_FORMAT = -3
DESIGNED = {c.name: c for c in ic.malformed_int() + ic.bool_cases()}


@pytest.fixture(scope="module")
def engine():
    eng = gs.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def host_checked(tmp_path_factory):
    cases = list(DESIGNED.values())
    run = ic.run_host_check(tmp_path_factory.mktemp("int_host"), cases,
                            sanitize=False)
    assert run is not None, "no host C++ compiler"
    res, ndec, nrej = run
    assert res.returncode == 0, res.stdout + res.stderr
    assert ("%d decoded pages, %d rejected pages, 0 failures"
            % (ndec, nrej)) in res.stdout
    assert nrej == sum(c.reason in (ic.FORMAT, ic.SHORT) for c in cases)


def _page(c):
    bitset = None if c.valid is None else np.packbits(
        np.asarray(c.valid, bool), bitorder="little")
    return gs.build_page(c.data, c.nrows, bitset)


def _groups(cases, slot0):
    """One group per case.  slot0: the case's page is the time page, with a
    dummy field behind it; else it is the field behind a plain time page
    (a time page with a null row is refused at upload, so time-encoded
    pages with nulls are decoded as a field column)."""
    ctype = {ic.TS: gs.CT_TIME, ic.I64: gs.CT_I64, ic.BOOL: gs.CT_BOOL}
    groups = []
    for i, c in enumerate(cases):
        n = c.nrows
        if slot0:
            groups.append((i, [(_page(c), gs.CT_TIME),
                               (gs.page_of(np.zeros(n), gs.CT_F64),
                                gs.CT_F64)]))
        else:
            ts = np.arange(n, dtype=np.int64) * 1000
            groups.append((i, [(gs.page_of(ts, gs.CT_TIME), gs.CT_TIME),
                               (_page(c), ctype[c.kind])]))
    return groups


def _decode(engine, cases, slot0):
    gset = engine.upload(_groups(cases, slot0))
    try:
        assert gset.rows == sum(c.nrows for c in cases)
        out = torch.zeros(gset.rows, device="cuda", dtype=torch.uint8
                          if cases[0].kind == ic.BOOL else torch.int64)
        dv = torch.full((gset.rows,), 7, dtype=torch.uint8, device="cuda")
        engine.decode(gset, 0 if slot0 else 1, out, dv)
        return out.cpu().numpy(), dv.cpu().numpy(), gset.row_offsets()
    finally:
        gset.free()


def _decode_and_check(engine, cases, slot0):
    host, hv, offs = _decode(engine, cases, slot0)
    for c, off in zip(cases, offs):
        values, valid = ic.expect(c)
        assert (host[off:off + c.nrows] == values).all(), c.name
        assert (hv[off:off + c.nrows] == valid).all(), f"{c.name} validity"


def _with_cuts(kind):
    """Every corpus page of the kind, and its cuts at len-1, len-8, len-9,
    11 and 10 bytes that the oracle decodes."""
    out = []
    for c, d in ic.pages():
        if ic.KIND[c.kind] != kind:
            continue
        n = len(c.values)
        out.append(ic.Case(c.name, kind, d, n))
        for L in sorted({len(d) - 1, len(d) - 8, len(d) - 9, 11, 10}):
            cut = ic.Case(f"{c.name}@cut{L}", kind, d[:L], n)
            if 0 <= L < len(d) and ic.expect(cut) is not None:
                out.append(cut)
    return out


def _first_null(c):
    valid = np.ones(c.nrows + 1, bool)
    valid[0] = False
    return c._replace(name=c.name + "@first_null", nrows=c.nrows + 1,
                      valid=valid)


@pytest.mark.parametrize("kind", [ic.TS, ic.I64], ids=["ts", "i64"])
def test_whole_and_cut_pages_decode_as_the_oracle(engine, kind):
    """All valid: k_rle_par, k_s8b_par, k_raw_par and, for what they do
    not take, k_seq_i64.  First row null: k_seq_i64 alone."""
    cases = _with_cuts(kind)
    assert len(cases) > 3 * len(cc.cases("ts" if kind == ic.TS else "i64"))
    _decode_and_check(engine, cases, slot0=kind == ic.TS)
    _decode_and_check(engine, [_first_null(c) for c in cases], slot0=False)


def test_bool_pages_decode_as_the_oracle(engine):
    """k_bool_par (all valid) and k_seq_bool (nulls, and the empty page)."""
    cases = [c for c in DESIGNED.values()
             if c.kind == ic.BOOL and c.reason is None and c.nrows]
    assert len(cases) == 4 * len(ic.BOOL_N)  # less bool_n0, plus the Null one
    _decode_and_check(engine, cases, slot0=False)


GOOD = {ic.TS: "ts_rle_scaler3", ic.I64: "i64_mixed", ic.BOOL: "bool_n9"}
REJECTED = ["ts_bad_rle_len3", "i64_bad_rle_varint_open", "ts_bad_s8b_plen7",
            "i64_bad_unc_plen11", "ts_bad_sub3", "i64_bad_enc9",
            "ts_bad_rle_negative", "ts_bad_unc_decreases", "ts_bad_s8b_wraps",
            "bool_bad_varint_open", "bool_bad_second_byte",
            "bool_bad_count_below_rows"]


def _good(kind):
    if kind == ic.BOOL:
        return DESIGNED[GOOD[kind]]
    return next(ic.Case(c.name, kind, d, len(c.values))
                for c, d in ic.pages() if c.name == GOOD[kind])


def _refused(engine, cases, slot0, reason):
    with pytest.raises(RuntimeError) as ei:
        _decode(engine, cases, slot0)
    assert f"({GS_ERR_FORMAT})" in str(ei.value), ei.value
    assert reason in str(ei.value), ei.value


@pytest.mark.parametrize("name", REJECTED)
def test_rejected_page_fails_with_its_message(engine, host_checked, name):
    bad = DESIGNED[name]
    good = _good(bad.kind)
    slot0 = bad.kind == ic.TS
    _refused(engine, [good, bad, good], slot0, bad.reason)
    _decode_and_check(engine, [good, good], slot0)


def _scan_groups(rng, cut=None):
    """Four groups of an RLE time page and a Gorilla page, 50 rows each;
    cut: the data of group 1's time page, or None to leave the group out.
    Returns the groups and, per group, (ts, [values])."""
    groups, truth = [], []
    for g in range(4):
        ts = cc.T0 + g * 10**6 + np.arange(50, dtype=np.int64) * 3000
        data = orc.encode_ts(ts)
        assert data[1] >> 4 == cc.RLE and len(data) == 12
        vp = gs.page_of(S.walk(rng, 50), gs.CT_F64)
        if g == 1:
            if cut is None:
                continue
            data = cut(data)
        else:
            truth.append((ts, [S.page_data(vp, 50, orc.decode_f64)]))
        groups.append((g, [(gs.build_page(data, 50), gs.CT_TIME),
                           (vp, gs.CT_F64)]))
    return groups, truth


CUTS = {"len3": lambda d: d[:3], "len10": lambda d: d[:10],
        "len11_varint_open": lambda d: d[:10] + b"\x80"}


@pytest.mark.parametrize("cut", CUTS, ids=list(CUTS))
def test_fused_scan_refuses_what_decode_refuses(engine, host_checked, cut):
    """k_spans_rle opens the fused scan on the time pages' headers; the
    malformed page is not the set's last."""
    data = CUTS[cut](ic.rle_page(ic.TS))
    assert ic.expect(ic.Case(cut, ic.TS, data, 50)) is None
    lo, hi = cc.T0, cc.T0 + 10**9
    groups, _ = _scan_groups(np.random.default_rng(5), CUTS[cut])
    sc = S.Scanner(engine, groups, 1)
    try:
        with pytest.raises(RuntimeError) as ei:
            sc.scan_sync(lo, hi)
        assert f"({GS_ERR_FORMAT})" in str(ei.value), ei.value
        assert ic.FORMAT in str(ei.value), ei.value
    finally:
        sc.free()
    groups, truth = _scan_groups(np.random.default_rng(5))
    sc = S.Scanner(engine, groups, 1)
    try:
        S.check(sc.scan_sync(lo, hi), S.expect(truth, 1, lo, hi), cut)
    finally:
        sc.free()


def test_bool_count_past_the_page_is_short(engine, host_checked):
    """64 rows, count 64, 3 bytes of bits, second of three pages: refused
    by k_bool_par (all valid) and by k_seq_bool (one null row)."""
    bad = DESIGNED["bool_bad_count64_bytes3"]
    bad_null = DESIGNED["bool_bad_count64_bytes3_null"]
    assert bad.data[:3] == bytes([10, 0x10, 64]) and len(bad.data) == 6
    assert bad.nrows == 64 and bad.valid is None
    assert bad_null.data == bad.data and bad_null.nrows == 65
    one_null = bad_null.valid
    rng = np.random.default_rng(9)
    honest = ic.Case("honest64", ic.BOOL,
                     orc.encode_bool(rng.integers(0, 2, 64).astype(np.uint8)),
                     64)
    side = _good(ic.BOOL)
    _refused(engine, [side, bad, side], False, ic.SHORT)
    _refused(engine, [side, bad_null, side], False, ic.SHORT)
    _decode_and_check(engine, [side, honest, side], False)
    _decode_and_check(engine, [side, honest._replace(nrows=65,
                                                     valid=one_null), side],
                      False)
