"""A designed corpus for the string block ENCODER (gs_encode_str on the
host, gs_encode_str_pages_dev on the device; one source,
cnosdb_amd/csrc/gs_str_enc.h).

Each case is rows of bytes-or-None plus what the encoder must make of them:
the element kinds its block shows under str_corpus.scan_kinds, and, where
the case is about one particular element, that element as (kind, length,
offset).  Expected bytes are never stored: they come from
oracle.pyoracle.encode_str, whose compressor is independent of
gs_encode_str.  The compressor's heuristics decide what an input yields, so
tests/test_str_enc_corpus_cpu.py holds every declaration against the
oracle's block; an input that does not produce what it declares is
redesigned, never redeclared.

The encoder can only ever emit lit0, lit1, lit2, copy1 and copy2: a
fragment is at most 65536 bytes, so a literal's length-1 fits two bytes and
a copy's offset fits two bytes.  lit3, lit4 and copy4 are unreachable, and
no case may show them (UNREACHABLE).

How the inputs steer the compressor:
  * the hash table starts as zeros, i.e. every empty slot names position 0
    of the fragment, and positions 1, 2, ... are entered one by one while
    no match has been found yet (32 probes at step 1 before the step grows);
  * behind a long incompressible stretch the step is large and a repeat is
    missed, but right behind an emitted copy the step is 1 again.  So a
    repeat that must be found stands directly behind a run of one byte
    (which is one long copy at offset 1): the run's match ends exactly where
    the repeat starts, and the very next table lookup is the repeat's first
    four bytes;
  * a match is extended as far as the bytes agree, so the byte behind the
    first occurrence differs from the byte behind the second.
"""
import collections

import numpy as np

EncCase = collections.namedtuple(
    "EncCase", "name rows kinds exact elements payload")
EncCase.__doc__ = """rows: bytes or None (null) per row; kinds: the kinds
scan_kinds must find (exact: and no others); elements: (kind, length,
offset-or-None) tuples that must occur in the stream; payload: the payload
size in bytes."""

REACHABLE = ("lit0", "lit1", "lit2", "copy1", "copy2")
UNREACHABLE = ("lit3", "lit4", "copy4")

RUN = b"\x00"  # the run byte; no other part of a steered input holds it


def varint_len(v):
    n = 1
    while v >= 0x80:
        n += 1
        v >>= 7
    return n


def payload_len(rows):
    return sum(len(s) + varint_len(len(s)) for s in rows if s is not None)


def noise(n, seed):
    """n bytes in 1..255, incompressible for every practical purpose."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 256, n, dtype=np.uint8).tobytes()


def distinct(n, start):
    """n <= 64 different bytes from `start` upwards (no 4-byte repeat)."""
    assert n <= 64 and start + n <= 256 and start > 0
    return bytes(range(start, start + n))


def text(n, seed):
    """n bytes of tag-like, well compressible text."""
    out, i = [], seed
    while sum(map(len, out)) < n:
        out.append(b"host_%d,region=eu-%d,rack=%d;" % (i % 97, i % 5, i % 11))
        i += 1
    return b"".join(out)[:n]


def one_string_of_payload(p, make):
    """A single string whose payload (varint + bytes) is exactly p."""
    for w in (1, 2, 3):
        if p - w >= 0 and varint_len(p - w) == w:
            return make(p - w)
    raise AssertionError(p)


def elements(data):
    """(kind, length, offset-or-None) of every element of a snappy block."""
    assert data[:2] == b"\x07\x10"
    s, i = data[2:], 0
    while s[i] >= 0x80:
        i += 1
    i += 1
    out = []
    while i < len(s):
        tag = s[i]
        i += 1
        if tag & 3 == 0:
            nb = max(0, (tag >> 2) - 59)
            n = (tag >> 2) if nb == 0 else int.from_bytes(s[i:i + nb],
                                                          "little")
            out.append(("lit%d" % nb, n + 1, None))
            i += nb + n + 1
        elif tag & 3 == 1:
            out.append(("copy1", 4 + ((tag >> 2) & 7), (tag >> 5) << 8 | s[i]))
            i += 1
        elif tag & 3 == 2:
            out.append(("copy2", (tag >> 2) + 1, s[i] | s[i + 1] << 8))
            i += 2
        else:
            out.append(("copy4", (tag >> 2) + 1,
                        int.from_bytes(s[i:i + 4], "little")))
            i += 4
    assert i == len(s)
    return out


def _case(name, rows, kinds, elems=()):
    """kinds: space-separated; a leading '=' declares that no other kind
    occurs."""
    exact = kinds.startswith("=")
    return EncCase(name, list(rows), frozenset(kinds.lstrip("=").split()),
                   exact, tuple(elems), payload_len(rows))


def _steered(head, gap, tail_start=0xC0):
    """One string: head, 4 separator bytes, a run of `gap` RUN bytes, head
    again, 20 closing bytes.  The second head is found as one match of
    len(head) bytes at offset len(head) + 4 + gap; head must not hold RUN,
    and the bytes behind its two occurrences differ."""
    assert RUN[0] not in head
    sep = distinct(4, 0xB0)
    return head + sep + RUN * gap + head + distinct(20, tail_start)


def _split(m):
    """The lengths a match of m bytes is cut into (codec: 64s while 68 or
    more are left, then 60 if more than 64 are left, then the rest)."""
    out = []
    while m >= 68:
        out.append(64)
        m -= 64
    if m > 64:
        out.append(60)
        m -= 60
    out.append(m)
    return out


def cases():
    out = []
    # -- the n >= 15 gate and the smallest payloads.  A payload of 0 bytes
    # does not exist with a string in it (an empty string is its length
    # byte); no strings at all is the empty block of the all-null page.
    out.append(_case("only_empty", [b""] * 3, "=lit0", [("lit0", 3, None)]))
    out.append(_case("all_null_rows", [None] * 5, "="))
    out.append(_case("payload_1", [b""], "=lit0", [("lit0", 1, None)]))
    for p in (14, 15, 16):
        s = distinct(p - 1, 0x41)
        out.append(_case("payload_%d" % p, [s], "=lit0", [("lit0", p, None)]))
    # -- every table size: 256 .. 16384 entries, at and one past the size.
    # The second half repeats the first behind a run, so the table is used.
    for tsz in (256, 512, 1024, 2048, 4096, 8192, 16384):
        for p in (tsz, tsz + 1):
            def make(n, tsz=tsz):
                head = noise(40, 1000 + tsz)
                body = _steered(head, 70)
                assert len(body) <= n
                return body + text(n - len(body), tsz)
            s = one_string_of_payload(p, make)
            out.append(_case("table_%d_payload_%d" % (tsz, p), [s],
                             "=lit0 copy1 copy2",
                             [("copy2", 40, 40 + 4 + 70)]))
    # -- fragment seams
    for p, last in ((65535, None), (65536, None), (65537, ("lit0", 1, None)),
                    (65536 + 14, ("lit0", 14, None)), (65536 + 15, None),
                    (131073, ("lit0", 1, None))):
        s = one_string_of_payload(p, lambda n: text(n, 3))
        out.append(_case("seam_payload_%d" % p, [s], "=lit0 copy1 copy2",
                         [last] if last else []))
    # -- literal length forms: one incompressible string, one literal
    for p, kind in ((60, "lit0"), (61, "lit1"), (256, "lit1"), (257, "lit2")):
        s = one_string_of_payload(p, lambda n: noise(n, 60 + p))
        out.append(_case("literal_%d" % p, [s], "=" + kind, [(kind, p, None)]))
    # -- a whole incompressible fragment and a bit: skip acceleration
    out.append(_case("incompressible_70000", [noise(69997, 7)], "=lit2",
                     [("lit2", 65536, None), ("lit2", 70000 - 65536, None)]))
    # -- copy1 against copy2: length 4, 11, 12 below and from offset 2048
    for ln in (4, 11, 12):
        for gap in (100, 2048):
            off = ln + 4 + gap
            kind = "copy1" if ln < 12 and off < 2048 else "copy2"
            head = distinct(ln, 0x61)
            out.append(_case("copy_len%d_off%d" % (ln, off),
                             [_steered(head, gap)], "lit0 " + kind,
                             [(kind, ln, off)]))
    # offset 2047 / 2048 exactly, length 4
    for off in (2047, 2048):
        out.append(_case("copy_len4_off%d" % off,
                         [_steered(distinct(4, 0x61), off - 8)],
                         "lit0 copy1" if off < 2048 else "lit0 copy2",
                         [("copy1" if off < 2048 else "copy2", 4, off)]))
    # -- the split of long matches
    for m in (64, 65, 67, 68, 69, 130):
        head = noise(m, 800 + m)
        off = m + 4 + 100
        elems = [("copy1" if ln < 12 else "copy2", ln, off)
                 for ln in _split(m)]
        out.append(_case("match_%d" % m, [_steered(head, 100)],
                         " ".join({"lit0", "lit1"} | {e[0] for e in elems}),
                         elems))
    # -- a match whose candidate is position 0 of the fragment: the first
    # four payload bytes come again at position 4, and the slot they hash
    # to is still empty, which reads as position 0
    out.append(_case("candidate_position_0", [b"abc"] * 8, "=lit0 copy2",
                     [("lit0", 4, None), ("copy2", 28, 4)]))
    # -- varint widths of the string length
    out.append(_case("varint_widths",
                     [b"", b"x", noise(127, 1), noise(128, 2),
                      noise(16383, 3), noise(16384, 4)], "=lit2"))
    # -- tag-like short strings, nulls in between
    tags = [b"host_%d" % (i % 7) for i in range(300)]
    out.append(_case("tags", tags, "lit0 copy1 copy2"))
    out.append(_case("tags_with_nulls",
                     [None if i % 5 == 2 else t for i, t in enumerate(tags)],
                     "lit0 copy1 copy2"))
    return out


_CACHE = []


def corpus():
    if not _CACHE:
        cs = cases()
        assert len({c.name for c in cs}) == len(cs)
        _CACHE.extend(cs)
    return list(_CACHE)


def page_layout(block, rows, crc32):
    """The page around a block (tsm/page.rs:488-497): header, crc over the
    data region, LSB-first bitset, block."""
    n = len(rows)
    valid = np.array([s is not None for s in rows], dtype=bool)
    bitset = np.packbits(valid, bitorder="little").tobytes()
    return (len(bitset).to_bytes(4, "big") + n.to_bytes(8, "big") +
            crc32(block).to_bytes(4, "big") + bitset + block)
