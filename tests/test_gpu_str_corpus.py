"""GPU string decode (gs_decode_str) over the designed snappy-stream corpus
(tests/str_corpus.py): every literal length form, every copy kind, the
overlap matrix, offsets past 64 KiB, Encoding::Null blocks and validity
patterns must decode to the corpus's declared rows, byte for byte; every
malformed page must fail the call, and the failure must not stick to the
engine.

k_str_decode runs the source of cnosdb_amd/csrc/gs_str_dec.h, which also
compiles as host C++.  No malformed page is uploaded before the host
program (tests/cpu/str_decode_check.cpp) has passed over the whole corpus
in this very run; test_str_decode_cpu.py runs the same program under
AddressSanitizer and UBSan."""
import numpy as np
import pytest
import torch

import cnosdb_amd as gs
import str_corpus as sc

pytestmark = pytest.mark.gpu

WF, MF = sc.corpus()


@pytest.fixture(scope="module")
def engine():
    eng = gs.Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def host_checked(tmp_path_factory):
    res = sc.run_host_check(tmp_path_factory.mktemp("str_host"), WF + MF,
                            sanitize=False)
    assert res is not None, "no host C++ compiler"
    assert res.returncode == 0, res.stdout + res.stderr
    assert ("%d well-formed pages, %d malformed pages, 0 failures"
            % (len(WF), len(MF))) in res.stdout


def _groups(cases):
    """One group per case: [time page, the case's string page]."""
    groups = []
    for i, c in enumerate(cases):
        ts = np.arange(c.nrows, dtype=np.int64) * 10**9
        bitset = None if c.valid is None else sc.bitset_of(c)
        groups.append((i, [(gs.page_of(ts, gs.CT_TIME), gs.CT_TIME),
                           (gs.build_page(c.data, c.nrows, bitset),
                            gs.CT_STR)]))
    return groups


def _expect(cases, row_off, rows):
    """Arrow offsets, bytes and validity bytes of the cases' rows."""
    lens = np.zeros(rows, np.int64)
    valid = np.zeros(rows, np.uint8)
    parts = [b""] * rows
    for c, base in zip(cases, row_off):
        for r, s in enumerate(c.rows):
            if s is not None:
                lens[base + r] = len(s)
                valid[base + r] = 1
                parts[base + r] = s
    off = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, b"".join(parts), valid


def _decode_and_check(engine, cases, caps=None):
    """Upload `cases` as one set and decode it once per capacity in `caps`
    (offsets from the exact total; default: exact), asserting everything
    decode_str returns."""
    gset = engine.upload(_groups(cases))
    rows = gset.rows
    assert rows == sum(c.nrows for c in cases)
    off, data, valid = _expect(cases, gset.row_offsets(), rows)
    total = len(data)
    try:
        for cap in caps or [total]:
            d_off = torch.full((rows + 1,), -1, dtype=torch.int64,
                               device="cuda")
            d_bytes = torch.zeros(max(cap, 0), dtype=torch.uint8,
                                  device="cuda")
            d_valid = torch.full((rows,), 7, dtype=torch.uint8, device="cuda")
            if cap < total:
                with pytest.raises(RuntimeError):
                    engine.decode_str(gset, 1, d_off, d_bytes, d_valid)
                continue
            got = engine.decode_str(gset, 1, d_off, d_bytes, d_valid)
            assert got == total
            assert (d_off.cpu().numpy() == off).all()
            assert d_bytes[:total].cpu().numpy().tobytes() == data
            assert (d_valid.cpu().numpy() == valid).all()
    finally:
        gset.free()


def test_well_formed_corpus_decodes_exactly(engine):
    total = sum(len(s) for c in WF for s in c.rows if s is not None)
    # roomy, one byte short (must raise), exact
    _decode_and_check(engine, WF, caps=[total + 64, total - 1, total])


GOOD = [c for c in WF if c.name in ("ends_on_literal", "set_nulls_first",
                                    "null_set_rows_11")]


@pytest.mark.parametrize("case", MF, ids=[c.name for c in MF])
def test_malformed_page_errors_and_engine_recovers(engine, host_checked,
                                                   case):
    assert len(GOOD) == 3
    gset = engine.upload(_groups([case, GOOD[0]]))
    rows = gset.rows
    d_off = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    d_bytes = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_valid = torch.zeros(rows, dtype=torch.uint8, device="cuda")
    try:
        with pytest.raises(RuntimeError):
            engine.decode_str(gset, 1, d_off, d_bytes, d_valid)
    finally:
        gset.free()
    # the device error flag is cleared: a good set decodes right after
    _decode_and_check(engine, GOOD)
