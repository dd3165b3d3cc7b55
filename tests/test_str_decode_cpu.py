"""The string page decoder of cnosdb_amd/csrc/gs_str_dec.h, run on the
host: the header k_str_decode and the upload's slab accounting share also
compiles as plain C++, so the snappy decompressor, the payload walk and the
slab size are exercised here under AddressSanitizer and UBSan by a
stand-alone program (tests/cpu/str_decode_check.cpp) over the whole designed
corpus (tests/str_corpus.py), malformed pages included, on buffers of
exactly the sizes the engine gives them."""
import pytest

import str_corpus as sc


def test_str_decode_host_sanitized(tmp_path):
    wf, mf = sc.corpus()
    res = sc.run_host_check(tmp_path, wf + mf, sanitize=True)
    if res is None:
        pytest.skip("no host C++ compiler")
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == ""  # the sanitizers stay silent
    assert ("%d well-formed pages, %d malformed pages, 0 failures"
            % (len(wf), len(mf))) in res.stdout
