"""Designed integer/timestamp inputs for the codec tests: every simple8b
selector, every timestamp scaler, the run-of-ones words, the small-n
rules, uncompressed pages and the shapes that cross a 256-word tile of
the block-parallel decoder.

Each case says what it is built to encode to (sub-encoding, scaler
nibble, exact selector set); test_codec_corpus_cpu.py holds the corpus to
those declarations with the oracle encoder, so a GPU test over the corpus
cannot pass on inputs that quietly became RLE or all-selector-15.

Built from numpy alone.  Not a test module and not a conftest."""
from collections import namedtuple

import numpy as np

UNCOMPRESSED, SIMPLE8B, RLE = 0, 1, 2

# values per word and bits per value of each selector (selectors 0 and 1
# are the runs of 240 / 120 ones and carry no payload)
S8B_COUNT = [240, 120, 60, 30, 20, 15, 12, 10, 8, 7, 6, 5, 4, 3, 2, 1]
S8B_WIDTH = [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 15, 20, 30, 60]

T0 = 1_700_000_000_000_000_000
I64_MIN, I64_MAX = -(2**63), 2**63 - 1

# kind: "ts" | "i64"; values: int64 array; sub: declared sub-encoding;
# scaler: declared low nibble of the sub-tag byte (0 for i64, which has
# none); selectors: exact set of selector nibbles of the simple8b words
# (empty unless sub == SIMPLE8B, and empty for a one-value block)
Case = namedtuple("Case", "name kind values sub scaler selectors")


def _u64(xs):
    return np.array([int(x) % (1 << 64) for x in xs], dtype=np.uint64)


def _zz_dec(z):
    z = int(z)
    return (z >> 1) ^ -(z & 1)


def ts_from_deltas(first, deltas, scale=1):
    """Timestamps whose packed simple8b values are `deltas` once the
    encoder has divided by `scale` (a power of ten)."""
    d = _u64([first] + [int(x) * scale for x in deltas])
    return np.cumsum(d, dtype=np.uint64).view(np.int64)


def i64_from_zz(first, zz):
    """Integers whose zigzagged deltas are `zz` (wrapping i64 sums)."""
    d = _u64([first] + [_zz_dec(z) for z in zz])
    return np.cumsum(d, dtype=np.uint64).view(np.int64)


def _from(kind, first, packed, scale=1):
    if kind == "ts":
        return ts_from_deltas(first, packed, scale)
    assert scale == 1
    return i64_from_zz(first, packed)


def _first(kind):
    return T0 if kind == "ts" else -12345


def _big(j, kind):
    """A packed value that fills a word alone (selector 15): at least
    2^30, all different so the page is not RLE, no multiple of ten so the
    timestamp scaler stays 0.  For i64 the zigzag parity alternates the
    sign, which keeps the running sum small."""
    return (1 << 40) + 2 * j + 1 if kind == "ts" else (1 << 40) + j


def selector_words(sel, reps=3):
    """`reps` words of selector `sel` (2..14): [2^w - 1, 0, 0, ...] fills
    exactly one word, since no narrower code holds 2^w - 1; the one value
    left at the end can only go into a selector-15 word.  Width 1 would be
    [1, 0, 0, ...] all the same; the alternating 1, 0 pattern keeps it away
    from RLE and from the run-of-ones detector alike."""
    w, c = S8B_WIDTH[sel], S8B_COUNT[sel]
    word = [1, 0] * (c // 2) if w == 1 else [(1 << w) - 1] + [0] * (c - 1)
    return word * reps + [(1 << w) - 1]


def _ones_shapes():
    """name -> (packed values, selectors).  The reference's own simple8b
    cases (240 ones, and the 120 / 119 / 239 splits) are raw word streams;
    as the deltas of a page, 240 equal deltas would be RLE, so that one
    shape carries one more, different delta at its end."""
    def changed(n, at):
        d = [1] * n
        d[at] = 5
        return d
    return {
        "ones240": ([1] * 240 + [3], {0, 15}),
        "ones240_at120": (changed(240, 120), {1, 2, 3, 4, 7}),
        "ones240_at119": (changed(240, 119), {2, 3, 4}),
        "ones241_at239": (changed(241, 239), {1, 2, 3, 4, 7, 15}),
        "ones360_then": ([1] * 360 + [9], {0, 1, 15}),
    }


def _mixed_packed():
    """Words of six widths, a 130-value run of ones in the middle and a
    lone wide value at the end."""
    p = []
    for sel in (3, 6, 9):
        p += selector_words(sel, reps=2)[:-1]
    p += [1] * 130
    for sel in (12, 13, 14):
        p += selector_words(sel, reps=2)[:-1]
    p += [(1 << 45) + 1]
    return p


def _cases(kind):
    out = []

    def add(name, values, sub, scaler=0, selectors=()):
        out.append(Case(f"{kind}_{name}", kind,
                        np.ascontiguousarray(values, dtype=np.int64), sub,
                        scaler, frozenset(selectors)))

    first = _first(kind)
    # one case per payload selector
    for sel in range(2, 15):
        add(f"sel{sel}", _from(kind, first, selector_words(sel)), SIMPLE8B,
            0, {sel, 15})
    # selector 15 at its widest: 2^59 <= packed < 2^60.  12 deltas keep a
    # timestamp below 2^63; the i64 deltas alternate in sign
    add("sel15_wide", _from(kind, 0, [(1 << 59) + 2 * j + 1 if kind == "ts"
                                      else (1 << 59) + j for j in range(12)]),
        SIMPLE8B, 0, {15})
    # run-of-ones words
    for name, (packed, sels) in _ones_shapes().items():
        add(name, _from(kind, first, packed), SIMPLE8B, 0, sels)
    # 256-word tiles of the block-parallel decoder: one value per word
    for nw in (255, 256, 257):
        add(f"tile_{nw}w", _from(kind, first,
                                 [_big(j, kind) for j in range(nw)]),
            SIMPLE8B, 0, {15})
    add("tile_sel0_then_300w",
        _from(kind, first, [1] * 240 + [_big(j, kind) for j in range(300)]),
        SIMPLE8B, 0, {0, 15})
    # the second tile starts with 4 one-value words, then the 240-run: its
    # carried row count differs from the first tile's
    add("tile_260w_then_sel0",
        _from(kind, first, [_big(j, kind) for j in range(260)] + [1] * 240),
        SIMPLE8B, 0, {0, 15})
    add("mixed", _from(kind, first, _mixed_packed()), SIMPLE8B, 0,
        {1, 3, 6, 7, 9, 12, 13, 14, 15})

    if kind == "ts":
        for k in range(13):
            step = 10**k
            # regular series, one missed stretch: 700 rows, 5 steps between
            # rows 400 and 401
            packed = [1] * 699
            packed[400] = 5
            add(f"gap_scaler{k}", ts_from_deltas(T0, packed, step), SIMPLE8B,
                k, {0, 1, 3, 4, 5, 12})
            add(f"rle_scaler{k}",
                T0 + np.arange(50, dtype=np.int64) * (3 * step), RLE, k)
        add("n1", [7], SIMPLE8B, 12)           # divisor loop never runs
        add("n2", [5, 1234567], RLE, 0)         # two rows are always RLE
        add("n2_scaler3", [5, 5 + 77000], RLE, 3)
        add("n3", [5, 12, 21], SIMPLE8B, 0, {14})
        add("uncompressed", [0, 1 << 61, (1 << 61) + 5, (1 << 62) + 5],
            UNCOMPRESSED)
        add("uncompressed_max", [3, I64_MAX - 1, I64_MAX], UNCOMPRESSED)
    else:
        # counter running down: 499 zigzagged deltas of 1, then +7
        vals = 10_000 - np.arange(500, dtype=np.int64)
        add("countdown500", np.concatenate([vals, [vals[-1] + 7]]), SIMPLE8B,
            0, {0, 5, 11})
        add("rle_const", np.full(50, -345632452354, dtype=np.int64), RLE)
        add("rle_step", I64_MAX - 10 - np.arange(60, dtype=np.int64) * 977,
            RLE)
        add("n1", [-7], SIMPLE8B)
        add("n2", [5, 1234567], SIMPLE8B, 0, {15})  # RLE needs three rows
        add("n3_rle", [5, 3, 1], RLE)
        add("n3", [5, 12, 21], SIMPLE8B, 0, {14})
        add("uncompressed", [0, 1 << 61, 0, -(1 << 61), 7], UNCOMPRESSED)
        # deltas that wrap across INT64_MIN / INT64_MAX
        add("uncompressed_wrap",
            [I64_MIN, 0, I64_MAX, I64_MIN, I64_MAX - 3, 7, I64_MIN],
            UNCOMPRESSED)
    return out


_CACHE = {}


def cases(kind):
    """The cases of one kind ("ts" or "i64"), built once; treat the arrays
    as read-only."""
    if kind not in _CACHE:
        cs = _cases(kind)
        for c in cs:
            c.values.setflags(write=False)
        _CACHE[kind] = cs
    return _CACHE[kind]


def case(name):
    for c in cases(name.split("_", 1)[0]):
        if c.name == name:
            return c
    raise KeyError(name)


# Pages whose declared row count disagrees with the values their data
# holds: (case name, declared rows).  Below: the decoder must stop early
# (the first one inside a run-of-ones word).  Above: rows past the last
# value are zero-filled.
ROW_MISMATCH = [
    ("ts_gap_scaler9", 150), ("ts_gap_scaler9", 731),
    ("ts_mixed", 140), ("ts_mixed", 420),
    ("i64_countdown500", 200), ("i64_countdown500", 533),
    ("i64_mixed", 140), ("i64_mixed", 420),
]


def selectors_of(block):
    """Selector nibbles of the simple8b words of an encoded ts/i64 block
    ([enc][sub|scaler][first BE64][words...])."""
    assert block[1] >> 4 == SIMPLE8B
    return {block[i] >> 4 for i in range(10, len(block), 8)}


def null_patterns(n):
    """name -> bool validity of a page that holds n values: the first row
    null, the last row null, and rows 0..7 null and no other (the bitset's
    first byte is zero)."""
    first = np.ones(n + 1, dtype=bool)
    first[0] = False
    last = np.ones(n + 1, dtype=bool)
    last[-1] = False
    byte0 = np.ones(n + 8, dtype=bool)
    byte0[:8] = False
    return {"first_null": first, "last_null": last, "byte0_null": byte0}
