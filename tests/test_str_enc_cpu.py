"""The string block encoder of cnosdb_amd/csrc/gs_str_enc.h, run on the
host with the device's loads: the header gs_encode_str and k_str_enc_pages
share also compiles as plain C++, so the payload framing and the snappy
compressor are exercised here under AddressSanitizer and UBSan by a
stand-alone program (tests/cpu/str_enc_check.cpp) over the whole designed
corpus (tests/str_enc_corpus.py), on buffers of exactly the sizes the header
states, with the oracle's blocks as the expected bytes."""
import os
import struct
import subprocess

import pytest

import str_corpus as sc
import str_enc_corpus as ec
from oracle import pyoracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "cpu", "str_enc_check.cpp")
INC = os.path.join(REPO, "cnosdb_amd", "csrc")


def _record(case):
    present = [s for s in case.rows if s is not None]
    block = orc.encode_str(present) if present else b""
    name = case.name.encode()
    return b"".join([
        struct.pack("<I", len(name)), name,
        struct.pack("<I", len(present)),
        b"".join(struct.pack("<Q", len(s)) for s in present),
        b"".join(present),
        struct.pack("<I", len(block)), block])


def test_str_enc_host_sanitized(tmp_path):
    cxx = sc.host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "str_enc_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + sc.SANITIZE +
                   ["-I", INC, SRC, "-o", exe], check=True)
    cases = ec.corpus()
    path = str(tmp_path / "str_enc_cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)) +
                b"".join(_record(c) for c in cases))
    res = subprocess.run([exe, path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == ""  # the sanitizers stay silent
    assert "%d cases, 0 failures" % len(cases) in res.stdout
