/* The Gorilla f64 bit-window parser (float.rs:351-606): the single home of
 * the stream format.  Every kernel that walks a Gorilla bitstream — the
 * upload pre-passes k_gor_sync / k_gor_sync_null and the chunked decodes
 * k_gor_chunks / k_gor_chunks_null — goes through the functions below; the
 * fused scan kernel k_gor_chunks_filtered takes its starting state from
 * gor_position and runs its own tuned refill and row loop.
 *
 * Page data: [enc=6][0x10][first f64 BE][bitstream] (float.rs:418-444).
 * Each further value is one of
 *   0                          repeat of the previous value
 *   10 <meaningful bits>       XOR with the previous value, same window
 *   11 <lead:5> <meaningful:6> <meaningful bits>      XOR, new window
 * where a 6-bit meaningful field of 0 stands for 64, and the stream ends
 * with the XOR value that yields GORILLA_SENTINEL.
 *
 * Budget accounting: instead of decrementing a bit budget per value (2
 * ops/value + 2 checks/value on the round-1 parser), the cursor advances
 * freely and correctness is enforced by
 * (a) a load clamp: words at/after p_clamp read as zero, so no access
 *     ever leaves the blob's 48-B tail pad;
 * (b) an overrun flag: once the window would hold only pad (entering
 *     word index >= W+2), `over` is set and the caller stops with
 *     DERR_SHORT — bounds every loop on corrupt input within ~128 pad bits;
 * (c) exact end checks, evaluated once per chunk (at the sentinel, or on
 *     completing a non-final chunk): gor_used_bits > total_bits means the
 *     parse ran past the real stream -> DERR_SHORT, reproducing the
 *     reference's "unexpected end of block" (float.rs:462) surface.
 *
 * Plain integer code, no atomics, LDS or lane intrinsics: raising errors
 * stays with the kernels, and the header also compiles as host C++
 * (tests/cpu/gor_window_check.cpp). */
#ifndef GS_GORILLA_H
#define GS_GORILLA_H

#include <cstdint>
#include "gs_internal.h"

#ifdef __HIPCC__
#define GOR_FN __host__ __device__ __forceinline__
#else
#define GOR_FN inline
#endif

/* Parser window state.  hi:lo is a 128-bit window holding nb valid bits,
 * left-aligned; nextw/nextw2 are the two words prefetched behind it. */
struct GorChunkState {
    const uint8_t *p;       /* next 8-byte word to prefetch */
    const uint8_t *stream;  /* bitstream start (page data + 10) */
    const uint8_t *p_clamp; /* loads at/after here read as zero */
    const uint8_t *p_over;  /* reaching here = stream overrun */
    uint64_t hi, lo, nextw, nextw2;
    uint64_t val;           /* bits of the previous value */
    int64_t total_bits;     /* bits the stream really holds */
    int nb;
    uint32_t trailing, meaningful; /* current XOR window */
    bool bad;  /* positioning failed: no header value, or a recorded state
                  at/after the stream end (poisoned); nothing else is set */
    bool over; /* a refill reached p_over */
};

GOR_FN uint64_t gor_be64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}

/* Positioning.  Both forms return whether the state is usable (= !bad);
 * they first derive the stream bounds and the load clamp from data_len. */
GOR_FN bool gor_bounds(GorChunkState &st, const uint8_t *data,
                       uint32_t data_len) {
    st.bad = false;
    st.over = false;
    if (data_len < 10) { st.bad = true; return false; }
    st.stream = data + 10;
    st.total_bits = int64_t(data_len - 10) * 8;
    uint64_t W = (uint64_t(st.total_bits) + 63) >> 6;
    st.p_clamp = st.stream + 8 * W + 24;
    st.p_over = st.stream + 8 * W + 40;
    return true;
}

/* the header value (row 0), an empty window and the stream's first two
 * words prefetched */
GOR_FN void gor_header(GorChunkState &st, const uint8_t *data) {
    st.val = gor_be64(data + 2);
    st.trailing = 0;
    st.meaningful = 64;
    st.hi = 0;
    st.lo = 0;
    st.nb = 0;
    st.nextw = gor_be64(st.stream);
    st.nextw2 = gor_be64(st.stream + 8);
    st.p = st.stream + 16;
}

/* Position at a page's start (the upload pre-passes). */
GOR_FN bool gor_start(GorChunkState &st, const uint8_t *data,
                      uint32_t data_len) {
    if (!gor_bounds(st, data, data_len)) return false;
    gor_header(st, data);
    return true;
}

/* Position at a chunk's start: the page header for the page's first chunk
 * (whose bitpos is 0 and val unset), else the state gor_record stored. */
GOR_FN void gor_position(GorChunkState &st, const uint8_t *blob,
                         const DevGorChunk &c) {
    const uint8_t *data = blob + c.data_off;
    if (!gor_bounds(st, data, c.data_len)) return;
    if (c.row0 == 0) {
        gor_header(st, data);
    } else {
        if (int64_t(c.bitpos) >= st.total_bits) { /* poisoned / truncated */
            st.bad = true;
            return;
        }
        st.val = c.val;
        st.trailing = c.trailing;
        st.meaningful = c.meaningful;
        const uint8_t *p = st.stream + (c.bitpos >> 6) * 8;
        unsigned rem = unsigned(c.bitpos & 63);
        uint64_t w0 = gor_be64(p);
        p += 8;
        st.hi = (rem == 0) ? w0 : (w0 << rem);
        st.lo = 0;
        st.nb = int(64 - rem);
        st.nextw = gor_be64(p);
        st.nextw2 = gor_be64(p + 8);
        st.p = p + 16;
    }
}

/* refill the window by one word; only with nb < 64 */
GOR_FN void gor_topup(GorChunkState &st) {
    uint64_t x = st.nextw;
    st.nextw = st.nextw2;
    st.over |= (st.p >= st.p_over);
    st.nextw2 = (st.p < st.p_clamp) ? gor_be64(st.p) : 0;
    st.p += 8;
    if (st.nb == 0) { st.hi = x; st.lo = 0; }
    else { st.hi |= x >> st.nb; st.lo = x << (64 - st.nb); }
    st.nb += 64;
}

/* drop the window's top k bits, k in 1..=64 */
GOR_FN void gor_consume(GorChunkState &st, unsigned k) {
    st.hi = (k == 64) ? st.lo : ((st.hi << k) | (st.lo >> (64 - k)));
    st.lo = (k == 64) ? 0 : (st.lo << k);
    st.nb -= int(k);
}

/* bits consumed from the stream start: words fetched minus the two staged
 * ahead, minus what the window still holds */
GOR_FN int64_t gor_used_bits(const GorChunkState &st) {
    return int64_t(st.p - st.stream) * 8 - 128 - st.nb;
}

/* Parse one value into st.val; needs nb >= 64 (gor_topup first).  Returns
 * whether it was an XOR value: only those can be the sentinel, a repeat of
 * a sentinel-valued row cannot.
 * Uniform path (no repeat/xor branch): a repeat is an XOR value with 0
 * meaningful bits (sb=0), so every lane runs the same straight-line code
 * and a wave diverges only on the rare need>=64 case — measured the
 * round-1 two-branch parse at ~20% VALU utilization, divergence being the
 * dominant loss. */
GOR_FN bool gor_parse(GorChunkState &st) {
    uint32_t top13 = uint32_t(st.hi >> 51);
    unsigned bit0 = (top13 >> 12) & 1; /* 1 = XOR value */
    unsigned bit1 = (top13 >> 11) & 1; /* 1 = new window */
    unsigned nw = bit0 & bit1;
    uint32_t lead = (top13 >> 6) & 0x1f;
    uint32_t mg_raw = top13 & 0x3f;
    uint32_t mg_new = mg_raw ? mg_raw : 64;
    uint32_t tr_new = mg_raw ? (64 - lead - mg_raw) : 0;
    st.meaningful = nw ? mg_new : st.meaningful;
    st.trailing = nw ? tr_new : st.trailing;
    unsigned shift = bit0 ? (bit1 ? 13u : 2u) : 1u;
    unsigned m_eff = bit0 ? st.meaningful : 0u;
    unsigned need = shift + m_eff; /* <= 77 */
    uint64_t sb;
    if (__builtin_expect(need < 64, 1)) {
        /* nb >= 64 on entry; need < 64 keeps the consume branch-free (no
           k==64 case) */
        uint64_t w = (st.hi << shift) | (st.lo >> (64 - shift));
        sb = m_eff ? (w >> ((64 - m_eff) & 63)) : 0;
        st.hi = (st.hi << need) | (st.lo >> (64 - need));
        st.lo <<= need;
        st.nb -= int(need);
    } else { /* m_eff >= 51: rare; two steps (topup needs nb < 64) */
        gor_consume(st, shift);
        while (st.nb < int(m_eff)) gor_topup(st);
        sb = (m_eff == 64) ? st.hi : (st.hi >> (64 - m_eff));
        gor_consume(st, m_eff);
    }
    st.val ^= sb << st.trailing;
    return bit0 != 0;
}

/* Upload pre-pass: store the state at a chunk boundary for gor_position. */
GOR_FN void gor_record(const GorChunkState &st, DevGorChunk &c) {
    c.bitpos = uint64_t(gor_used_bits(st));
    c.val = st.val;
    c.trailing = uint8_t(st.trailing);
    c.meaningful = uint8_t(st.meaningful);
}

/* Upload pre-pass: mark a chunk whose state could not be recorded.  A
 * bitpos past the stream end (data_len = the page's) makes gor_position
 * report bad, so the decode of that chunk raises DERR_SHORT; the window is
 * the neutral one. */
GOR_FN void gor_poison(DevGorChunk &c, uint32_t data_len) {
    c.bitpos = uint64_t(data_len) * 8;
    c.val = 0;
    c.trailing = 0;
    c.meaningful = 64;
    c.flags = 0;
}

#endif
