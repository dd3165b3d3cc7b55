"""The designed string corpus (tests/str_corpus.py) is what it says it is:
every page holds exactly the element kinds it declares, the plain Python
decoder and the oracle both decode it to the declared rows or reject it,
and the corpus covers every form the decoder distinguishes.  The product
encoder is tied to the same Python decoder, which was not derived from
it."""
import numpy as np
import pytest

import cnosdb_amd as gs
import str_corpus as sc
from oracle import pyoracle as orc

WF, MF = sc.corpus()


def _ids(cases):
    return [c.name for c in cases]


def _valid(c):
    return None if c.valid is None else list(c.valid)


def test_corpus_names_are_unique_and_pages_small():
    names = _ids(WF + MF)
    assert len(set(names)) == len(names)
    # only offsets and literals past 64 KiB need a page that long
    big = [c.name for c in WF + MF if len(c.data) > 40000]
    assert all(("6553" in n or "70000" in n) for n in big), big
    assert all(len(c.data) <= 64 for c in MF)


def test_corpus_covers_every_element_kind():
    seen = set()
    for c in WF:
        seen |= c.kinds
    assert seen == set(sc.KINDS)
    reasons = {c.reject for c in MF}
    assert reasons == {sc.PREAMBLE, sc.HEADER, sc.ENCODING, sc.OFFSET_ZERO,
                       sc.OFFSET_RANGE, sc.OVERRUN, sc.TRUNCATED,
                       sc.SHORT_OUTPUT, sc.LEN_VARINT, sc.LEN_PREFIX,
                       sc.LEN_RANGE}


def test_declared_kinds_match_tag_scan():
    wrong = [c.name for c in WF + MF if sc.scan_kinds(c.data) != c.kinds]
    assert wrong == []


def test_well_formed_decodes_to_declared_rows():
    wrong = []
    for c in WF:
        assert c.reject is None and len(c.rows) == c.nrows, c.name
        if sc.decode_page(c.data, c.nrows, _valid(c)) != c.rows:
            wrong.append(("python", c.name))
        if orc.decode_str(c.data, c.nrows, _valid(c)) != c.rows:
            wrong.append(("oracle", c.name))
    assert wrong == []


@pytest.mark.parametrize("case", MF, ids=_ids(MF))
def test_malformed_is_rejected_for_declared_reason(case):
    assert case.rows is None
    with pytest.raises(sc.Reject) as ei:
        sc.decode_page(case.data, case.nrows, _valid(case))
    assert ei.value.reason == case.reject
    with pytest.raises(RuntimeError):
        orc.decode_str(case.data, case.nrows, _valid(case))


def _encoder_inputs():
    """The string sets of the GPU string tests (test_gpu_strings.py), with
    the same generator and seeds."""
    rng = np.random.default_rng(29)
    tags = [b"hostname=host_%04d" % i for i in range(64)]
    sets = []
    for t in range(8):
        n = int(rng.integers(1, 3000))
        sets.append([tags[int(rng.integers(0, 64))] if rng.random() < 0.6
                     else bytes(rng.integers(0, 256, int(rng.integers(0, 60)))
                                .astype(np.uint8)) for _ in range(n)])
        if t % 2:
            rng.random(n)
    sets.append([b""] * 37)
    sets.append([bytes(rng.integers(97, 123, 60).astype(np.uint8))
                 for _ in range(2500)])  # > 64 KiB: more than one fragment
    sets.append([b"hello world, this is a longer string"] * 50)
    rng2 = np.random.default_rng(77)
    tagpool = [b"host_%06d" % i for i in range(64)]
    sets.append([tagpool[i] for i in rng2.integers(0, 64, 4000)])
    sets.append([b"alpha", b"", b"\x00\xff weird", b"tail"])
    return sets


def test_product_encoder_decodes_through_python_decoder():
    for k, strings in enumerate(_encoder_inputs()):
        blk = gs.encode_str(strings)
        assert sc.decode_page(blk, len(strings)) == strings, k
        # the encoder emits no 4-byte offsets: only the designed corpus
        # takes a decoder there
        assert "copy4" not in sc.scan_kinds(blk), k
