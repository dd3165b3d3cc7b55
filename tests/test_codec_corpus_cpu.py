"""The designed codec corpus (codec_corpus.py) against its own
declarations, on the CPU.  The GPU tests over the corpus mean what they
say only while every case still encodes to the words it was built for;
this module is that condition.  Bytes come from the oracle encoder; the
host encoder must agree with it on every case."""
import numpy as np
import pytest

import cnosdb_amd as gs
import codec_corpus as cc
from oracle import pyoracle as orc

ORC_ENC = {"ts": orc.encode_ts, "i64": orc.encode_i64}
HOST_ENC = {"ts": gs.encode_ts, "i64": gs.encode_i64}
ENC_BYTE = {"ts": 11, "i64": 2}  # DeltaTs, Delta
ALL = cc.cases("ts") + cc.cases("i64")


@pytest.fixture(scope="module")
def blocks():
    return {c.name: ORC_ENC[c.kind](c.values) for c in ALL}


def test_case_names_unique():
    assert len({c.name for c in ALL}) == len(ALL)


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_case_encodes_as_declared(c, blocks):
    b = blocks[c.name]
    assert b[0] == ENC_BYTE[c.kind]
    assert b[1] >> 4 == c.sub
    assert b[1] & 0x0F == c.scaler
    if c.sub == cc.SIMPLE8B:
        assert (len(b) - 10) % 8 == 0
        assert cc.selectors_of(b) == set(c.selectors)
    else:
        assert not c.selectors


@pytest.mark.parametrize("c", ALL, ids=lambda c: c.name)
def test_host_encoder_equals_oracle_and_roundtrips(c, blocks):
    b = blocks[c.name]
    assert HOST_ENC[c.kind](c.values) == b
    assert (orc.decode_i64(b, c.values.size) == c.values).all()


@pytest.mark.parametrize("kind", ["ts", "i64"])
def test_union_covers_all_16_selectors(kind, blocks):
    seen = set()
    for c in cc.cases(kind):
        if c.sub == cc.SIMPLE8B:
            seen |= cc.selectors_of(blocks[c.name])
    assert seen == set(range(16))


@pytest.mark.parametrize("sub", [cc.SIMPLE8B, cc.RLE])
def test_union_covers_all_13_ts_scalers(sub, blocks):
    seen = {blocks[c.name][1] & 0x0F for c in cc.cases("ts")
            if blocks[c.name][1] >> 4 == sub}
    assert seen == set(range(13))
    if sub == cc.SIMPLE8B:
        # and each of them on a page that has run-of-ones words
        runs = {blocks[c.name][1] & 0x0F for c in cc.cases("ts")
                if blocks[c.name][1] >> 4 == sub
                and {0, 1} <= cc.selectors_of(blocks[c.name])}
        assert runs == set(range(13))


def test_tile_cases_straddle_256_words(blocks):
    """The word counts the tile-carry cases are named for."""
    for kind in ("ts", "i64"):
        words = {c.name: (len(blocks[c.name]) - 10) // 8
                 for c in cc.cases(kind)}
        for nw in (255, 256, 257):
            assert words[f"{kind}_tile_{nw}w"] == nw
        assert words[f"{kind}_tile_sel0_then_300w"] == 301
        assert words[f"{kind}_tile_260w_then_sel0"] == 261
        b = blocks[f"{kind}_tile_sel0_then_300w"]
        assert b[10] >> 4 == 0            # the run word comes first
        b = blocks[f"{kind}_tile_260w_then_sel0"]
        assert b[-8] >> 4 == 0            # ... and here last, in tile two


def test_row_mismatch_pages_truncate_and_zero_fill(blocks):
    """What the GPU test expects of a page whose row count disagrees with
    its data: fewer rows stop the decode early, more rows are zero."""
    for name, nrows in cc.ROW_MISMATCH:
        c = cc.case(name)
        n = c.values.size
        assert nrows != n
        got = orc.decode_i64(blocks[name], nrows)
        m = min(n, nrows)
        assert (got[:m] == c.values[:m]).all()
        assert (got[m:] == 0).all()
    below = [nrows for name, nrows in cc.ROW_MISMATCH
             if nrows < cc.case(name).values.size]
    assert len(below) == len(cc.ROW_MISMATCH) // 2
    # the run-of-ones pages are cut inside their first (240-run) word
    for name in ("ts_gap_scaler9", "i64_countdown500"):
        assert blocks[name][10] >> 4 == 0
        assert min(r for nm, r in cc.ROW_MISMATCH if nm == name) < 240


def test_null_patterns_shape():
    p = cc.null_patterns(20)
    assert all(int(v.sum()) == 20 for v in p.values())
    assert not p["first_null"][0] and p["first_null"][1:].all()
    assert not p["last_null"][-1] and p["last_null"][:-1].all()
    assert np.packbits(p["byte0_null"], bitorder="little")[0] == 0
    assert p["byte0_null"][8:].all()
