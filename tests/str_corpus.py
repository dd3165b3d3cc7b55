"""Designed string pages for the string decode tests: snappy raw streams
built element by element (every literal length form, every copy kind,
overlapping copies, offsets past 64 KiB), the Encoding::Null form, validity
patterns, and one-element-wrong malformed neighbours of those.

The product encoder emits no 4-byte-offset copy, no copy shorter than 4
bytes and no offset above 65535, so pages it produced cannot reach those
decoder branches; these can.  Each case says what it holds (the exact set
of element kinds) and what it must decode to, or why it must be rejected;
test_str_corpus_cpu.py holds the corpus to those declarations.

`decode_page` is a plain reference decoder written from the snappy format
description and codec/string.rs:226-309: unbounded Python ints, one byte at
a time, derived from neither C decoder of this project.  Expected rows of
the cases do not come from it either: they are the strings the case was
built from, with copies expanded in closed form (`_repeat`).

Left out on purpose, because the verdict depends on choices private to the
reference's snappy and varint libraries: non-canonical varints, a tenth
varint byte above 1, UTF-8 validity (the engine is varbinary).

numpy and the standard library only.  Not a test module and not a
conftest."""
import os
import shutil
import struct
import subprocess
from collections import namedtuple

import numpy as np

SNAPPY_HDR = b"\x07\x10"  # Encoding::Snappy, STRING_COMPRESSED_SNAPPY << 4
NULL_HDR = b"\x01"        # Encoding::Null

# element kinds: lit0 = literal with the length in the tag, lit1..lit4 =
# literal with a 1..4-byte length field, copy1/2/4 by offset width
KINDS = ("lit0", "lit1", "lit2", "lit3", "lit4", "copy1", "copy2", "copy4")

# reasons for rejection
PREAMBLE = "preamble does not end"
HEADER = "no room for the block header"
ENCODING = "unknown encoding byte"
OFFSET_ZERO = "copy offset 0"
OFFSET_RANGE = "copy reaches before the output's start"
OVERRUN = "element overruns the declared length"
TRUNCATED = "stream ends inside an element"
SHORT_OUTPUT = "output shorter than the declared length"
LEN_VARINT = "string length varint does not end within 10 bytes"
LEN_PREFIX = "fewer than 8 bytes left for a length prefix"
LEN_RANGE = "string longer than the rest of the payload"
SHORT_PAYLOAD = "payload used up with valid rows left"

# name; data = the page's data region; nrows; valid = tuple of bools or None
# (every row valid); kinds = exact set of element kinds in the stream;
# rows = expected values (bytes, None for a null row) or None when the page
# must be rejected; reject = the reason, or None
Case = namedtuple("Case", "name data nrows valid kinds rows reject")


class Reject(Exception):
    def __init__(self, reason):
        super().__init__(reason)
        self.reason = reason


# ------------------------------------------------------------ builders

def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7f) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def literal(data, len_field_bytes=None):
    """Literal element holding `data`.  len_field_bytes: None = shortest
    form, 0 = in the tag, 1..4 = that many length bytes."""
    n = len(data) - 1
    if len_field_bytes is None:
        len_field_bytes = 0 if n < 60 else (n.bit_length() + 7) // 8
    if len_field_bytes == 0:
        assert 0 <= n < 60
        return bytes([n << 2]) + data
    assert 0 <= n < 1 << (8 * len_field_bytes)
    return (bytes([(59 + len_field_bytes) << 2]) +
            n.to_bytes(len_field_bytes, "little") + data)


def copy1(off, length):
    assert 4 <= length <= 11 and 0 <= off < 2048
    return bytes([1 | ((length - 4) << 2) | ((off >> 8) << 5), off & 0xff])


def copy2(off, length):
    assert 1 <= length <= 64 and 0 <= off < 1 << 16
    return bytes([2 | ((length - 1) << 2)]) + off.to_bytes(2, "little")


def copy4(off, length):
    assert 1 <= length <= 64 and 0 <= off < 1 << 32
    return bytes([3 | ((length - 1) << 2)]) + off.to_bytes(4, "little")


COPY = {"copy1": copy1, "copy2": copy2, "copy4": copy4}


def block(stream, ulen):
    """Snappy string block: header, preamble `ulen`, the elements."""
    return SNAPPY_HDR + varint(ulen) + stream


def payload(strings):
    return b"".join(varint(len(s)) + s for s in strings)


def null_payload(strings):
    return b"".join(len(s).to_bytes(8, "big") + s for s in strings)


def null_block(strings):
    """Encoding::Null block (string.rs:169-183)."""
    return NULL_HDR + null_payload(strings)


def _repeat(out, off, n):
    """What a copy of n bytes from `off` back appends to `out`."""
    assert 0 < off <= len(out)
    return (out[-off:] * (n // off + 1))[:n]


def _noise(n, seed):
    """n bytes with no period, so that a wrong offset shows."""
    return np.random.default_rng(seed).integers(0, 256, n).astype(
        np.uint8).tobytes()


DISTINCT = bytes(range(0x41, 0x51))  # 16 different bytes


# ------------------------------------------------------- reference decoder

def _read_varint(buf, i, reason):
    """(value, next index) of the LEB128 integer at buf[i:]."""
    v = 0
    for k in range(10):
        if i + k >= len(buf):
            raise Reject(reason)
        b = buf[i + k]
        v |= (b & 0x7f) << (7 * k)
        if b < 0x80:
            return v, i + k + 1
    raise Reject(reason)


def snappy_decompress(stream):
    ulen, i = _read_varint(stream, 0, PREAMBLE)
    out = bytearray()
    n = len(stream)
    while i < n:
        tag = stream[i]
        i += 1
        kind = tag & 3
        if kind == 0:
            length = (tag >> 2) + 1
            if length > 60:
                nb = length - 60
                if i + nb > n:
                    raise Reject(TRUNCATED)
                length = 1 + sum(stream[i + k] << (8 * k) for k in range(nb))
                i += nb
            if len(out) + length > ulen:
                raise Reject(OVERRUN)
            if i + length > n:
                raise Reject(TRUNCATED)
            for k in range(length):
                out.append(stream[i + k])
            i += length
            continue
        if kind == 1:
            if i + 1 > n:
                raise Reject(TRUNCATED)
            length = 4 + ((tag >> 2) & 7)
            off = ((tag >> 5) << 8) | stream[i]
            i += 1
        else:
            nb = 2 if kind == 2 else 4
            if i + nb > n:
                raise Reject(TRUNCATED)
            length = (tag >> 2) + 1
            off = sum(stream[i + k] << (8 * k) for k in range(nb))
            i += nb
        if off == 0:
            raise Reject(OFFSET_ZERO)
        if off > len(out):
            raise Reject(OFFSET_RANGE)
        if len(out) + length > ulen:
            raise Reject(OVERRUN)
        for _ in range(length):
            out.append(out[-off])
    if len(out) != ulen:
        raise Reject(SHORT_OUTPUT)
    return bytes(out)


def decode_page(data, nrows, valid=None):
    """Rows of a string page: bytes, or None for a null row.  Raises Reject.
    Where the payload is used up while valid rows remain the reference
    returns a shorter array; this project rejects the page."""
    if len(data) == 0:
        return [None] * nrows
    if data[0] == 7:
        if len(data) < 2:
            raise Reject(HEADER)
        pl = snappy_decompress(data[2:])
        be = False
    elif data[0] == 1:
        pl = data[1:]
        be = True
    else:
        raise Reject(ENCODING)
    rows, i = [], 0
    for r in range(nrows):
        if valid is not None and not valid[r]:
            rows.append(None)
            continue
        if i >= len(pl):
            raise Reject(SHORT_PAYLOAD)
        if be:
            if i + 8 > len(pl):
                raise Reject(LEN_PREFIX)
            slen = int.from_bytes(pl[i:i + 8], "big")
            i += 8
        else:
            slen, i = _read_varint(pl, i, LEN_VARINT)
        if i + slen > len(pl):
            raise Reject(LEN_RANGE)
        rows.append(bytes(pl[i:i + slen]))
        i += slen
    return rows


def scan_kinds(data):
    """Element kinds a tag scan of a snappy block finds.  The scan stops
    where an element runs off the stream; a literal that does still counts."""
    found = set()
    if len(data) < 2 or data[0] != 7:
        return found
    s = data[2:]
    i = 0
    while i < len(s) and s[i] >= 0x80:
        i += 1
    i += 1
    while i < len(s):
        tag = s[i]
        i += 1
        if tag & 3 == 0:
            nb = max(0, (tag >> 2) - 59)
            found.add("lit%d" % nb)
            if i + nb > len(s):
                break
            n = (tag >> 2) if nb == 0 else int.from_bytes(s[i:i + nb],
                                                          "little")
            i += nb + n + 1
        else:
            found.add(("copy1", "copy2", "copy4")[(tag & 3) - 1])
            i += (1, 2, 4)[(tag & 3) - 1]
    return found


# ------------------------------------------------------------ the corpus

def _single(name, kinds, plan, lit_field=None):
    """A page of one string, built from a plan of elements: ("lit", bytes)
    or (copy kind, offset, length).  The first element must be a literal;
    the string's length varint is put in front of its bytes.  An offset of
    "all" means everything produced so far."""
    sizes = [len(p[1]) if p[0] == "lit" else p[2] for p in plan]
    vi = varint(sum(sizes))
    out, raw = b"", b""
    for k, p in enumerate(plan):
        if p[0] == "lit":
            d = (vi if k == 0 else b"") + p[1]
            raw += literal(d, lit_field if k == 0 else None)
            out += d
        else:
            off = len(out) if p[1] == "all" else p[1]
            raw += COPY[p[0]](off, p[2])
            out += _repeat(out, off, p[2])
    assert plan[0][0] == "lit" and out[:len(vi)] == vi
    return Case(name, block(raw, len(out)), 1, None, frozenset(kinds.split()),
                [out[len(vi):]], None)


def _lit_total(total):
    """Body of the one-string payload whose only literal is `total` long."""
    for n in (total - 1, total - 2, total - 3):
        if n >= 0 and n + len(varint(n)) == total:
            return _noise(n, total)
    raise AssertionError(total)


def _strings(name, strings, valid, kinds="", null_enc=False, extra=()):
    """A page of many strings in one literal (or Encoding::Null): one per
    valid row, then `extra` strings that no row takes."""
    nrows = len(strings)
    present = [s for r, s in enumerate(strings)
               if valid is None or valid[r]] + list(extra)
    rows = [s if valid is None or valid[r] else None
            for r, s in enumerate(strings)]
    if null_enc:
        data = null_block(present)
    else:
        pl = payload(present)
        data = block(literal(pl), len(pl))
    return Case(name, data, nrows, None if valid is None else tuple(valid),
                frozenset(kinds.split()), rows, None)


STRING_SETS = [
    # every width of the length varint
    ("widths", [b"", b"a", _noise(127, 1), _noise(128, 2), _noise(16383, 3),
                _noise(16384, 4)], None, "lit2"),
    ("nulls_first", [b"x", b"y", b"first", b"", b"last"],
     [False, False, True, True, True], "lit0"),
    ("nulls_last", [b"first", b"", b"last", b"x", b"y"],
     [True, True, True, False, False], "lit0"),
    # 11 rows: the last validity byte is partly used
    ("rows_11", [b"r%d" % r for r in range(11)],
     [r % 3 != 1 for r in range(11)], "lit0"),
]


def well_formed():
    cs = []
    # literal length forms
    for total in (1, 60, 61, 256, 257, 65536, 65537):
        nb = 0 if total <= 60 else ((total - 1).bit_length() + 7) // 8
        cs.append(_single("lit_len_%d" % total, "lit%d" % nb,
                          [("lit", _lit_total(total))]))
    cs.append(_single("lit_field4_small", "lit4", [("lit", DISTINCT)],
                      lit_field=4))
    for total in range(8, 24):  # word-copy tails
        cs.append(_single("lit_tail_%d" % total, "lit0",
                          [("lit", _lit_total(total))]))
    # copies by kind; the literal in front is just long enough for the
    # offset, which decides the form of its length field
    head_kind = {2047: "lit2 ", 2048: "lit2 ", 65535: "lit3 ", 65536: "lit3 ",
                 70000: "lit3 "}
    for length in (4, 11):
        for off in (1, 7, 8, 9, 2047):
            cs.append(_single(
                "copy1_len%d_off%d" % (length, off),
                "lit0 " + head_kind.get(off, "") + "copy1",
                [("lit", _noise(max(off, 16), off)), ("copy1", off, length),
                 ("lit", b"tail")]))
    for length in (1, 3, 64):
        for off in (1, 8, 2048, 65535):
            cs.append(_single(
                "copy2_len%d_off%d" % (length, off),
                "lit0 " + head_kind.get(off, "") + "copy2",
                [("lit", _noise(max(off, 16), off)), ("copy2", off, length),
                 ("lit", b"tail")]))
    # 70000 catches a decoder that drops the high offset bytes
    for off in (5, 65536, 70000):
        cs.append(_single(
            "copy4_off%d" % off, "lit0 " + head_kind.get(off, "") + "copy4",
            [("lit", _noise(max(off, 16), off)), ("copy4", off, 37),
             ("lit", b"tail")]))
    # overlap matrix: offset 1..16 x length {1..24, 64} behind 16 distinct
    # bytes; offsets below 8 repeat a pattern, the others may go by words
    for off in range(1, 17):
        for length in list(range(1, 25)) + [64]:
            cs.append(_single("overlap_off%d_len%d" % (off, length),
                              "lit0 copy2",
                              [("lit", DISTINCT), ("copy2", off, length)]))
    # offset = everything produced so far, the length varint included
    cs.append(_single("copy_from_start", "lit0 copy2",
                      [("lit", DISTINCT), ("copy2", "all", 17)]))
    cs.append(_single("copy4_from_start", "lit0 copy4",
                      [("lit", DISTINCT), ("copy4", "all", 64)]))
    # last element ends exactly at the declared length
    cs.append(_single("ends_on_copy", "lit0 copy1",
                      [("lit", DISTINCT), ("copy1", 4, 8)]))
    cs.append(_single("ends_on_literal", "lit0 copy1",
                      [("lit", DISTINCT), ("copy1", 4, 8), ("lit", b"tail.")]))
    # string sets, as snappy and as Encoding::Null blocks
    for name, strings, valid, kinds in STRING_SETS:
        cs.append(_strings("set_" + name, strings, valid, kinds))
        cs.append(_strings("null_set_" + name, strings, valid, null_enc=True))
    cs.append(Case("all_null_empty", b"", 13, (False,) * 13, frozenset(),
                   [None] * 13, None))
    # more strings than valid rows: the tail is ignored
    cs.append(_strings("extra_strings", [b"one", b"nil", b"two"],
                       [True, False, True], "lit0", extra=[b"unused", b""]))
    cs.append(_strings("null_extra_strings", [b"one", b"nil", b"two"],
                       [True, False, True], null_enc=True,
                       extra=[b"unused", b""]))
    return cs


def _bad(name, kinds, data, reason, nrows=1, valid=None):
    return Case(name, data, nrows, valid, frozenset(kinds.split()), None,
                reason)


def malformed():
    """One-element-wrong variants of the page
        literal(varint + 16 distinct bytes), copy(offset 4, length 8),
        literal("tail.")
    which is the well-formed case ends_on_literal."""
    body_len = 16 + 8 + 5
    head = varint(body_len) + DISTINCT  # 17 bytes of output
    ulen = len(head) + 8 + 5
    lit_h, lit_t = literal(head), literal(b"tail.")
    cs = []
    for kind, mk in COPY.items():
        k = "lit0 " + kind
        # M1: offset 0
        cs.append(_bad("m1_offset0_" + kind, k,
                       block(lit_h + mk(0, 8) + lit_t, ulen), OFFSET_ZERO))
        # M2: offset one past what has been produced; copy as first element
        cs.append(_bad("m2_offset_past_" + kind, k,
                       block(lit_h + mk(len(head) + 1, 8) + lit_t, ulen),
                       OFFSET_RANGE))
        cs.append(_bad("m2_copy_first_" + kind, k,
                       block(mk(1, 8) + lit_h + lit_t, ulen), OFFSET_RANGE))
        # M3: the copy overruns the declared length by 1
        cs.append(_bad("m3_copy_overrun_" + kind, k,
                       block(lit_h + mk(4, 8), ulen - 5 - 1), OVERRUN))
    good = lit_h + copy1(4, 8)
    cs.append(_bad("m3_literal_overrun", "lit0 copy1",
                   block(good + literal(b"tail.!"), ulen), OVERRUN))
    # M4: the stream ends inside an element
    cs.append(_bad("m4_cut_literal_length", "lit0 lit2 copy1",
                   block(good + b"\xf4\x04", ulen), TRUNCATED))
    cs.append(_bad("m4_cut_literal_body", "lit0 copy1",
                   block(good + lit_t[:-1], ulen), TRUNCATED))
    cs.append(_bad("m4_cut_copy1", "lit0 copy1",
                   block(lit_h + copy1(4, 8)[:1], ulen), TRUNCATED))
    cs.append(_bad("m4_cut_copy2", "lit0 copy2",
                   block(lit_h + copy2(4, 8)[:2], ulen), TRUNCATED))
    cs.append(_bad("m4_cut_copy4", "lit0 copy4",
                   block(lit_h + copy4(4, 8)[:4], ulen), TRUNCATED))
    # M5: every element is whole, the output one byte short
    cs.append(_bad("m5_output_short", "lit0 copy1",
                   block(good + literal(b"tail"), ulen), SHORT_OUTPUT))
    # M6: a literal of 2^32 bytes between elements that add up
    cs.append(_bad("m6_literal_2pow32", "lit0 lit4",
                   block(lit_h + b"\xfc\xff\xff\xff\xff" + copy1(4, 8) + lit_t,
                         ulen), OVERRUN))
    # M7: preambles
    cs.append(_bad("m7_preamble_lone_80", "", SNAPPY_HDR + b"\x80", PREAMBLE))
    cs.append(_bad("m7_preamble_ten_80", "", SNAPPY_HDR + b"\x80" * 10,
                   PREAMBLE))
    cs.append(_bad("m7_preamble_minus1", "lit0 copy1",
                   block(good + lit_t, ulen - 1), OVERRUN))
    for nm, v in (("plus1", ulen + 1), ("2pow32", 1 << 32),
                  ("2pow63", 1 << 63), ("2pow64_minus16", (1 << 64) - 16)):
        cs.append(_bad("m7_preamble_" + nm, "lit0 copy1",
                       block(good + lit_t, v), SHORT_OUTPUT))
    # M8: length prefixes in the payload, behind one good string
    first = varint(5) + b"hello"

    def pl_case(name, pl, reason, nrows=2):
        kinds = "lit0" if len(pl) <= 60 else "lit1"
        cs.append(_bad(name, kinds, block(literal(pl), len(pl)), reason,
                       nrows))
    pl_case("m8_varint_runs_off", first + b"\x80", LEN_VARINT)
    pl_case("m8_len_remaining_plus1", first + varint(3) + b"ab", LEN_RANGE)
    pl_case("m8_len_2pow64_minus1", first + b"\xff" * 9 + b"\x01", LEN_RANGE)
    pl_case("m8_varint_11_bytes", first + b"\x80" * 10 + b"\x00" + b"pad",
            LEN_VARINT)
    be_first = (5).to_bytes(8, "big") + b"hello"
    cs.append(_bad("m8_be_prefix_cut", "", NULL_HDR + be_first + bytes(7),
                   LEN_PREFIX, 2))
    cs.append(_bad("m8_be_len_remaining_plus1", "",
                   NULL_HDR + be_first + (3).to_bytes(8, "big") + b"ab",
                   LEN_RANGE, 2))
    cs.append(_bad("m8_be_len_2pow64_minus1", "",
                   NULL_HDR + be_first + b"\xff" * 8 + b"ab", LEN_RANGE, 2))
    # M9, M10
    cs.append(_bad("m9_unknown_encoding", "",
                   b"\x7f" + block(good + lit_t, ulen)[1:], ENCODING))
    cs.append(_bad("m10_only_encoding_byte", "", b"\x07", HEADER))
    cs.append(_bad("m10_only_header", "", SNAPPY_HDR, PREAMBLE))
    return cs


_CACHE = {}


def corpus():
    """(well-formed cases, malformed cases), built once."""
    if not _CACHE:
        _CACHE["wf"], _CACHE["mf"] = well_formed(), malformed()
    return _CACHE["wf"], _CACHE["mf"]


def bitset_of(case):
    """Packed LSB-first validity bytes of a case."""
    v = np.ones(case.nrows, bool) if case.valid is None else np.array(
        case.valid, bool)
    return np.packbits(v, bitorder="little")


# ------------------------------------------------- host check of the header

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(REPO, "tests", "cpu", "str_decode_check.cpp")
CHECK_INC = os.path.join(REPO, "cnosdb_amd", "csrc")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def host_compiler():
    for cxx in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def write_cases_file(path, cases):
    """The input of tests/cpu/str_decode_check.cpp (little-endian):
      u32 ncases
      per case: u32 name_len, name; u32 data_len, data; u32 nrows;
                u32 all_valid; (nrows+7)/8 validity bytes; u32 reject;
                u64 payload_len (the decoded payload; 0 for a reject);
                per row (unless reject): i64 len (-1 = null), then the
                bytes of all rows back to back"""
    out = [struct.pack("<I", len(cases))]
    for c in cases:
        nm = c.name.encode()
        out.append(struct.pack("<I", len(nm)) + nm)
        out.append(struct.pack("<I", len(c.data)) + c.data)
        out.append(struct.pack("<II", c.nrows, int(c.valid is None)))
        out.append(bitset_of(c).tobytes())
        out.append(struct.pack("<I", int(c.rows is None)))
        if c.rows is None:
            out.append(struct.pack("<Q", 0))
            continue
        if c.data[:1] == b"\x07":
            plen = len(snappy_decompress(c.data[2:]))
        else:
            plen = max(0, len(c.data) - 1)
        out.append(struct.pack("<Q", plen))
        out.append(b"".join(struct.pack("<q", -1 if s is None else len(s))
                            for s in c.rows))
        out.append(b"".join(s for s in c.rows if s is not None))
    with open(path, "wb") as f:
        f.write(b"".join(out))


def run_host_check(workdir, cases, sanitize, verbose=False):
    """Build tests/cpu/str_decode_check.cpp in `workdir` and run it over
    `cases`.  Returns the finished process, or None without a compiler."""
    cxx = host_compiler()
    if cxx is None:
        return None
    exe = os.path.join(str(workdir), "str_decode_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g"] +
                   (SANITIZE if sanitize else []) +
                   ["-I", CHECK_INC, CHECK_SRC, "-o", exe], check=True)
    path = os.path.join(str(workdir), "str_cases.bin")
    write_cases_file(path, cases)
    return subprocess.run([exe, path] + (["-v"] if verbose else []),
                          capture_output=True, text=True)
