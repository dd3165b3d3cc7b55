"""The integer and bool page decoders of cnosdb_amd/csrc/gs_int_dec.h, run
on the host: the header the decode kernels, k_spans_rle and the upload
share also compiles as plain C++, so int_page_header, int_page_decode and
bool_page_decode are exercised here by a stand-alone program
(tests/cpu/int_decode_check.cpp) under AddressSanitizer and UBSan, on
buffers of exactly the pages' sizes: over the designed corpus at every row
count and null pattern, every prefix truncation of every corpus page, and
the designed malformed pages (tests/int_corpus.py).  Expectations are the
oracle's."""
import re

import pytest

import codec_corpus as cc
import int_corpus as ic


def _summary(ndec, nrej):
    return "%d decoded pages, %d rejected pages, 0 failures" % (ndec, nrej)


def test_designed_pages_are_what_they_claim():
    """The oracle refuses exactly the designed pages declared FORMAT or
    SHORT, and the malformed list covers every rule."""
    designed = ic.malformed_int() + ic.bool_cases()
    names = [c.name for c in designed]
    assert len(set(names)) == len(names)
    wrong = [c.name for c in designed
             if (ic.expect(c) is None) != (c.reason in (ic.FORMAT, ic.SHORT))]
    assert wrong == []
    for k in ("ts", "i64"):
        have = {c.name for c in designed if c.name.startswith(k + "_bad_")}
        want = ([f"rle_len{L}" for L in range(3, 11)]
                + ["rle_varint_open", "rle_varint_11"]
                + [f"s8b_plen{p}" for p in range(8)]
                + ["unc_plen0", "unc_plen11"]
                + [f"sub{s}" for s in range(3, 16)]
                + ["enc0", "enc3", "enc6", "enc7", "enc9", "enc10", "enc12",
                   "enc255", "one_byte", "raw_short_word", "rle_negative",
                   "unc_decreases", "s8b_wraps"])
        assert {f"{k}_bad_{w}" for w in want} <= have
    assert ([c.name for c in designed if c.reason == ic.NONMONO]
            == ["ts_bad_rle_negative", "ts_bad_unc_decreases",
                "ts_bad_s8b_wraps"])


def test_int_decode_host_sanitized(tmp_path):
    """No case is skipped or filtered: the program's summary carries the
    number of cases written."""
    trunc = ic.truncation_cases()
    assert len(trunc) == sum(len(d) for _, d in ic.pages())
    cases = (ic.decode_cases() + trunc + ic.malformed_int() + ic.bool_cases())
    run = ic.run_host_check(tmp_path, cases, sanitize=True)
    if run is None:
        pytest.skip("no host C++ compiler")
    res, ndec, nrej = run
    assert ndec + nrej == len(cases)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert res.stderr == ""  # the sanitizers stay silent
    assert _summary(ndec, nrej) in res.stdout


def test_header_decoder_against_corpus_values(tmp_path):
    """The corpus declarations and the header's decoder, tied on the CPU:
    every corpus page decodes to the case's own values (not the oracle's
    decode), and int_page_header gives min_pos_delta's inputs, first and
    rle_delta, for every timestamp scaler."""
    cases = ic.value_cases()
    expected = [(c.values, [1] * len(c.values)) for c, _ in ic.pages()]
    run = ic.run_host_check(tmp_path, cases, sanitize=False,
                            expected=expected)
    if run is None:
        pytest.skip("no host C++ compiler")
    res, ndec, nrej = run
    assert (ndec, nrej) == (len(cases), 0)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert _summary(ndec, 0) in res.stdout
    hdr = {m[1]: (int(m[2]), int(m[3])) for m in
           re.finditer(r"^hdr (\S+) (-?\d+) (-?\d+)$", res.stdout, re.M)}
    assert hdr == {f"ts_rle_scaler{k}": (cc.T0, 3 * 10**k)
                   for k in range(13)}
