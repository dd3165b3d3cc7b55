"""Pages for the host and GPU checks of the integer and bool decoders
(cnosdb_amd/csrc/gs_int_dec.h): the designed corpus of codec_corpus.py as
encoded pages, at every row count and null pattern the codec tests use;
every prefix truncation of those pages; designed malformed pages, one per
rule of int_page_header and bool_page_header; and bool pages around the
byte and word sizes.

What a page must decode to comes from the oracle (pyoracle.decode_i64 /
decode_bool), never from the decoder under test.  The oracle has no
non-monotonic verdict and no validity output, so those two are declared
here: NONMONO only for the three pages designed for it, and a row valid
exactly when its validity bit is set, except that a Null-encoded page
nulls the valid rows it has no value for.

Built from numpy alone.  Not a test module and not a conftest."""
import os
import struct
import subprocess
from collections import namedtuple

import numpy as np

import codec_corpus as cc
from oracle import pyoracle as orc
from str_corpus import SANITIZE, host_compiler

TS, I64, BOOL = 0, 1, 2
KIND = {"ts": TS, "i64": I64, "bool": BOOL}
ENC = {TS: 11, I64: 2}  # DeltaTs, Delta
FORMAT, SHORT, NONMONO = "malformed", "shorter", "non-monotonic"

# kind: TS | I64 | BOOL; valid: bool array or None (all valid); reason:
# None, or what the page is designed to be refused for (the word of the
# engine's message); print_header: the host program prints first / rle_delta
Case = namedtuple("Case", "name kind data nrows valid reason print_header",
                  defaults=(None, None, False))


def _encode(c):
    return (orc.encode_ts if c.kind == "ts" else orc.encode_i64)(c.values)


_PAGES = []


def pages():
    """(corpus case, its encoded page) for every ts and i64 corpus case."""
    if not _PAGES:
        _PAGES.extend((c, _encode(c))
                      for c in cc.cases("ts") + cc.cases("i64"))
    return _PAGES


def value_cases():
    """Every corpus page at its own row count; expectation: c.values."""
    return [Case(c.name, KIND[c.kind], d, len(c.values),
                 print_header=c.name.startswith("ts_rle_scaler"))
            for c, d in pages()]


def decode_cases():
    """Every corpus page at its own row count, at each ROW_MISMATCH row
    count and under each null pattern."""
    out = value_cases()
    by_name = {c.name: (c, d) for c, d in pages()}
    for name, rows in cc.ROW_MISMATCH:
        c, d = by_name[name]
        out.append(Case(f"{name}@rows{rows}", KIND[c.kind], d, rows))
    for c, d in pages():
        for pat, valid in cc.null_patterns(len(c.values)).items():
            out.append(Case(f"{c.name}@{pat}", KIND[c.kind], d, len(valid),
                            valid))
    return out


def truncation_cases():
    """data[:L] of every corpus page, 0 <= L < len, all valid."""
    return [Case(f"{c.name}@cut{L}", KIND[c.kind], d[:L], len(c.values))
            for c, d in pages() for L in range(len(d))]


def _be(v):
    return struct.pack(">Q", v % (1 << 64))


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _zz(v):
    return ((v << 1) ^ (v >> 63)) % (1 << 64)


def _hdr(kind, sub, scaler=0):
    return bytes([ENC[kind], (sub << 4) | scaler])


def rle_page(kind, first=cc.T0, delta=3, count=50):
    """[enc][0x20][first BE64][varint delta][varint count]: 12 bytes."""
    if kind == I64:
        first, delta = _zz(first), _zz(delta)
    return (_hdr(kind, cc.RLE) + _be(first) + _varint(delta % (1 << 64)) +
            _varint(count))


def malformed_int():
    """Designed pages, one per rule of int_page_header and the row checks;
    the same byte layouts for ts and i64."""
    out = []
    for kind, k in ((TS, "ts"), (I64, "i64")):
        def add(name, data, nrows, reason=FORMAT, valid=None):
            out.append(Case(f"{k}_bad_{name}", kind, bytes(data), nrows,
                            valid, reason))
        rle = rle_page(kind)
        assert len(rle) == 12
        for L in range(3, 11):  # the varint starts at byte 10
            add(f"rle_len{L}", rle[:L], 50)
        add("rle_varint_open", rle[:10] + b"\x83", 50)
        add("rle_varint_11", rle[:10] + b"\x80" * 11, 50)
        for plen in range(8):
            add(f"s8b_plen{plen}", _hdr(kind, cc.SIMPLE8B) + bytes(plen), 5,
                SHORT)
        add("unc_plen0", _hdr(kind, cc.UNCOMPRESSED), 2)
        add("unc_plen11", _hdr(kind, cc.UNCOMPRESSED) + _be(8) + b"\0\0\1", 2)
        for sub in range(3, 16):
            add(f"sub{sub}", _hdr(kind, sub) + bytes(16), 2)
        for enc in (0, 3, 6, 7, 9, 10, 12, 255):  # not Null, Delta, DeltaTs
            add(f"enc{enc}", bytes([enc, 0x20]) + rle[2:], 50)
        add("one_byte", bytes([ENC[kind]]), 2)
        # decodes: the third row has no whole word and comes out null
        add("raw_short_word", b"\x01" + _be(5) + _be(6) + bytes(7), 3, None)
        # Backwards: refused as non-monotonic on a time column only.  An
        # RLE delta of -3, an uncompressed delta of -1, and a simple8b
        # delta (one 60-bit value per word) that carries past INT64_MAX.
        mono = NONMONO if kind == TS else None
        add("rle_negative", rle_page(kind, delta=-3), 50, mono)
        add("unc_decreases",
            _hdr(kind, cc.UNCOMPRESSED) + _be(100 if kind == TS else _zz(100))
            + _be(-1 if kind == TS else _zz(-1)), 2, mono)
        add("s8b_wraps",
            _hdr(kind, cc.SIMPLE8B)
            + _be(cc.I64_MAX - 1 if kind == TS else _zz(cc.I64_MAX - 1))
            + _be((15 << 60) | (5 if kind == TS else _zz(5))), 2, mono)
    return out


BOOL_N = (0, 1, 7, 8, 9, 63, 64, 65)


def bool_page(count, bits):
    """[10][0x10][varint count][bits]"""
    return bytes([10, 0x10]) + _varint(count) + bytes(bits)


def bool_cases():
    rng = np.random.default_rng(64)
    out = []
    for n in BOOL_N:
        data = orc.encode_bool(rng.integers(0, 2, n).astype(np.uint8))
        out.append(Case(f"bool_n{n}", BOOL, data, n))
        for pat, valid in cc.null_patterns(n).items():
            out.append(Case(f"bool_n{n}@{pat}", BOOL, data, len(valid), valid))
    noise = bytes(rng.integers(0, 256, 8).astype(np.uint8))
    one_null = np.ones(65, bool)
    one_null[9] = False
    # the count promises more bits than the page carries
    for nbytes in (0, 1, 3, 7):
        out.append(Case(f"bool_bad_count64_bytes{nbytes}", BOOL,
                        bool_page(64, noise[:nbytes]), 64, None, SHORT))
    out.append(Case("bool_bad_count64_bytes3_null", BOOL,
                    bool_page(64, noise[:3]), 65, one_null, SHORT))
    out.append(Case("bool_bad_count_2p40", BOOL, bool_page(1 << 40, noise),
                    65, None, SHORT))
    out.append(Case("bool_bad_count_below_rows", BOOL,
                    bool_page(10, noise[:3]), 20, None, SHORT))
    out.append(Case("bool_bad_varint_open", BOOL,
                    bytes([10, 0x10, 0x80, 0x80]), 4, None, FORMAT))
    out.append(Case("bool_bad_second_byte", BOOL,
                    bytes([10, 0x20]) + _varint(8) + noise[:1], 8, None,
                    FORMAT))
    # decodes: rows past the bytes present come out null
    out.append(Case("bool_null_enc_short", BOOL, bytes([1, 1, 0, 1]), 5))
    return out


# -------------------------------------------------------------- expectation

def expect(case):
    """(values, validity) the page must decode to, or None where the
    oracle refuses it."""
    dec = orc.decode_bool if case.kind == BOOL else orc.decode_i64
    try:
        values = dec(case.data, case.nrows, case.valid)
    except RuntimeError:
        return None
    valid = (np.ones(case.nrows, bool) if case.valid is None
             else np.asarray(case.valid, bool))
    if not case.data:
        valid = np.zeros(case.nrows, bool)
    elif case.data[0] == 1:  # Null encoding: one value per valid row
        avail = (len(case.data) - 1) // (1 if case.kind == BOOL else 8)
        valid = valid & (np.cumsum(valid) <= avail)
    return values.astype(np.int64), valid.astype(np.uint8)


# ------------------------------------------------- host check of the header

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(REPO, "tests", "cpu", "int_decode_check.cpp")
CHECK_INC = os.path.join(REPO, "cnosdb_amd", "csrc")


def write_cases_file(path, cases, expected=None):
    """The input of tests/cpu/int_decode_check.cpp (its header comment has
    the layout).  expected[i] overrides the oracle's expectation of case i.
    Returns (pages to decode, pages to reject)."""
    ndec = nrej = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for i, c in enumerate(cases):
            exp = expected[i] if expected else expect(c)
            nm = c.name.encode()
            bits = np.packbits(np.ones(c.nrows, bool) if c.valid is None
                               else np.asarray(c.valid, bool),
                               bitorder="little")
            flags = (int(exp is None) | 2 * int(c.reason == NONMONO)
                     | 4 * int(c.print_header))
            f.write(struct.pack("<I", len(nm)) + nm
                    + struct.pack("<II", c.kind, len(c.data)) + c.data
                    + struct.pack("<II", c.nrows, int(c.valid is None))
                    + bits.tobytes() + struct.pack("<I", flags))
            if exp is None:
                nrej += 1
                continue
            ndec += 1
            f.write(np.ascontiguousarray(exp[0], "<i8").tobytes()
                    + np.ascontiguousarray(exp[1], np.uint8).tobytes())
    return ndec, nrej


def run_host_check(workdir, cases, sanitize, expected=None):
    """Build tests/cpu/int_decode_check.cpp in `workdir` and run it over
    `cases`.  Returns (finished process, pages to decode, pages to reject),
    or None without a compiler."""
    cxx = host_compiler()
    if cxx is None:
        return None
    exe = os.path.join(str(workdir), "int_decode_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g"] +
                   (SANITIZE if sanitize else []) +
                   ["-I", CHECK_INC, CHECK_SRC, "-o", exe], check=True)
    path = os.path.join(str(workdir), "int_cases.bin")
    ndec, nrej = write_cases_file(path, cases, expected)
    res = subprocess.run([exe, path], capture_output=True, text=True)
    os.remove(path)  # the truncation sweep is tens of megabytes
    return res, ndec, nrej
