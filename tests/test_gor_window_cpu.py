"""The Gorilla window parser of cnosdb_amd/csrc/gs_gorilla.h, run on the
host: the header the GPU kernels share also compiles as plain C++, so its
positioning, refill, parse and bit accounting are exercised here under
AddressSanitizer and UBSan by a stand-alone program
(tests/cpu/gor_window_check.cpp), on pages from the product encoder with
the oracle's decode as the expected values."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import cnosdb_amd as gs
from oracle import pyoracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpu", "gor_window_check.cpp")
INC = os.path.join(REPO, "cnosdb_amd", "csrc")
PAD = 48  # zero bytes the engine's blob keeps behind the last page

NVALS = 300


def _host_compiler():
    for cxx in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def _pages():
    """(values, cut) per page; cut pages keep 60 % of their bytes."""
    rng = np.random.default_rng(20251021)
    walk = np.round(np.clip(np.cumsum(rng.normal(0, 0.5, NVALS)) + 50,
                            0, 100), 1)
    alternating = np.where(np.arange(NVALS) % 2 == 0, 0x3FF0000000000001,
                           0xBFF0000000000000).astype(np.uint64)
    return [
        (walk, False),
        (np.full(NVALS, 42.5), False),
        # all mantissa bits in use: 51 and more meaningful bits per value,
        # the parser's two-step path
        (rng.uniform(0, 1e3, NVALS), False),
        # 64 meaningful bits: the 6-bit length field holds 0
        (alternating.view(np.float64), False),
        (np.array([3.25]), False),
        (walk, True),
    ]


def _pages_file(path):
    blob = [struct.pack("<I", len(_pages()))]
    for vals, cut in _pages():
        data = gs.encode_f64(vals)
        exp = orc.decode_f64(data, len(vals)).view(np.uint64)
        assert exp.tolist() == np.asarray(vals).view(np.uint64).tolist()
        if cut:
            data = data[:int(len(data) * 0.6)]
        blob.append(struct.pack("<III", len(vals), len(data), int(cut)))
        blob.append(data + bytes(PAD))
        blob.append(exp.astype("<u8").tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(blob))


def test_gor_window_host_sanitized(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gor_window_check")
    subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe],
        check=True)
    pages = str(tmp_path / "pages.bin")
    _pages_file(pages)
    res = subprocess.run([exe, pages], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "5 whole pages, 1 cut pages, 0 failures" in res.stdout
