"""Holds the string-encoder corpus (tests/str_enc_corpus.py) to its
declarations: the oracle's block of every case shows the declared element
kinds and elements, decodes back to the rows through the plain Python
reference decoder of tests/str_corpus.py, and gs_encode_str gives the same
bytes."""
import pytest

import cnosdb_amd as gs
import str_corpus as sc
import str_enc_corpus as ec
from oracle import pyoracle as orc

CASES = ec.corpus()
IDS = [c.name for c in CASES]


def _present(case):
    return [s for s in case.rows if s is not None]


def _block(case):
    present = _present(case)
    return orc.encode_str(present) if present else b""


def test_corpus_reaches_what_the_issue_lists():
    payloads = {c.payload for c in CASES}
    want = {0, 1, 14, 15, 16, 65535, 65536, 65537, 65536 + 14, 65536 + 15,
            131073}
    for tsz in (256, 512, 1024, 2048, 4096, 8192, 16384):
        want |= {tsz, tsz + 1}
    assert want <= payloads, sorted(want - payloads)
    lens = {len(s) for c in CASES for s in c.rows if s is not None}
    assert {0, 1, 127, 128, 16383, 16384} <= lens
    seen = set()
    for c in CASES:
        seen |= sc.scan_kinds(_block(c))
    assert seen == set(ec.REACHABLE)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_declaration_holds(case):
    block = _block(case)
    kinds = sc.scan_kinds(block)
    assert not kinds & set(ec.UNREACHABLE)
    if case.exact:
        assert kinds == case.kinds
    else:
        assert case.kinds <= kinds
    if block:
        els = ec.elements(block)
        for e in case.elements:
            assert e in els, (e, els[:8], els[-4:])
    else:
        assert case.payload == 0 and not case.elements


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_block_round_trips(case):
    valid = [s is not None for s in case.rows]
    assert sc.decode_page(_block(case), len(case.rows), valid) == case.rows


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_encoder_equals_oracle(case):
    present = _present(case)
    assert gs.encode_str(present) == _block(case)
    page = gs.str_page_of([s or b"" for s in case.rows],
                          [s is not None for s in case.rows])
    assert page == ec.page_layout(_block(case), case.rows, orc.crc32)
