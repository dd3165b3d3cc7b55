"""The write-side codecs of cnosdb_amd/csrc/gs_tsm_enc.h, run on the host:
the header the encode kernels share with gs_encode.cpp also compiles as
plain C++, so the code the device runs (packing straight from the column,
the validity-skipping Gorilla loop, one bool byte at a time) is exercised
here under AddressSanitizer and UBSan by a stand-alone program
(tests/cpu/tsm_enc_check.cpp), with the oracle's encoders and CRC as the
expected bytes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import codec_corpus as corpus
from oracle import pyoracle as orc
from test_gor_window_cpu import _host_compiler, _pages

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpu", "tsm_enc_check.cpp")
INC = os.path.join(REPO, "cnosdb_amd", "csrc")

K_TS, K_I64, K_F64, K_BOOL = 0, 1, 2, 3
SENTINEL = 0x7ff8000000000ff
ERR_SENTINEL = -1  # TSM_ENC_ERR_SENTINEL

BOOL_N = (1, 7, 8, 9, 127, 128, 129)


def _case(kind, vals, expect, valid=None):
    """One record of the program's input; expect: the oracle's block, or a
    negative error code."""
    block = expect if isinstance(expect, bytes) else b""
    n = len(vals)
    out = [struct.pack("<IIIiI", kind, n, int(valid is not None),
                       len(block) if isinstance(expect, bytes) else expect,
                       orc.crc32(block)),
           struct.pack(">IQI", (n + 7) // 8, n, orc.crc32(block)),
           np.ascontiguousarray(vals).tobytes()]
    if valid is not None:
        out.append(np.asarray(valid, dtype=np.uint8).tobytes())
    out.append(block)
    return b"".join(out)


def _f64_valid_cases():
    """(values, validity): null slots hold values that must not be read as
    such, the sentinel among them."""
    rng = np.random.default_rng(20261021)
    n = 300
    walk = np.round(np.cumsum(rng.normal(0, 0.5, n)) + 50, 1)
    out = []
    for valid in (rng.random(n) < 0.7,                 # scattered nulls
                  np.arange(n) > 0,                    # first row null
                  np.arange(n) < n - 1,                # last row null
                  np.arange(n) >= 9,                   # bitset byte 0 null
                  np.arange(n) == 17,                  # one value
                  np.zeros(n, dtype=bool)):            # all null: no block
        vals = walk.copy()
        vals.view(np.uint64)[~valid] = SENTINEL
        out.append((vals, valid))
    return out


def _cases():
    recs = []
    for kind, name in ((K_TS, "ts"), (K_I64, "i64")):
        enc = orc.encode_ts if kind == K_TS else orc.encode_i64
        for c in corpus.cases(name):
            recs.append(_case(kind, c.values, enc(c.values)))
    for vals, cut in _pages():
        if not cut:  # the cut page is the walk again
            recs.append(_case(K_F64, np.asarray(vals, dtype=np.float64),
                              orc.encode_f64(vals)))
    for vals, valid in _f64_valid_cases():
        recs.append(_case(K_F64, vals, orc.encode_f64(vals[valid]), valid))
    rng = np.random.default_rng(7)
    for n in BOOL_N:
        vals = rng.integers(0, 2, n).astype(np.uint8)
        recs.append(_case(K_BOOL, vals, orc.encode_bool(vals)))
    # the sentinel as an input value behind the first: the oracle refuses
    # it, the encoder returns its error code
    bad = np.array([1.5, 2.5, 0.0, 3.5])
    bad.view(np.uint64)[2] = SENTINEL
    with pytest.raises(AssertionError):
        orc.encode_f64(bad)
    recs.append(_case(K_F64, bad, ERR_SENTINEL))
    return recs


def test_tsm_enc_host_sanitized(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "tsm_enc_check")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        check=True)
    recs = _cases()
    nint = len(corpus.cases("ts")) + len(corpus.cases("i64"))
    assert len(recs) == nint + 5 + 6 + len(BOOL_N) + 1
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    # every ts/i64 case is encoded twice (see the program's header)
    assert (f"{len(recs)} cases, {len(recs) + nint} encodes, 0 failures"
            in res.stdout)
