/* The TSM DataBlock encoders and the page header: the single home of the
 * write-side codecs.  The host entry points of gs_encode.cpp and the device
 * kernels k_enc_prepare / k_enc_group_pages of gs_engine.cpp all go through
 * the functions below, so a page encoded on the host and one encoded on the
 * device are the same code's output.
 *
 * Block layouts (reference: tskv/src/tsm/codec/; pinned by the InfluxDB
 * golden blocks, integer.rs:438-483, and the boolean vectors,
 * boolean.rs:156-181).  An empty input is an empty block.
 *
 *   ts   timestamp.rs:51-122   [11][sub<<4 | scaler][first u64 BE] ...
 *   i64  integer.rs:40-96      [2][sub<<4][zigzag(first) BE] ...
 *     The values behind the first are the wrapping deltas, raw for ts and
 *     zigzagged for i64 (u64 columns are the i64 codec over the same bits,
 *     unsigned.rs:15-18).
 *       sub 2  RLE: all deltas equal: [varint delta][varint count].  ts takes
 *              it from 2 rows on and counts the first value; i64 needs 3 rows
 *              and counts the deltas only.
 *       sub 0  uncompressed, when a delta needs more than 60 bits: every
 *              delta as u64 BE.
 *       sub 1  simple8b words, u64 BE each (simple8b.rs:26-76): selector in
 *              the top 4 bits; 0 and 1 are runs of 240 / 120 ones without
 *              payload, 2..15 hold TSM_S8B {count, bits} values, first value
 *              lowest.
 *     ts only: RLE and simple8b divide the deltas by the largest power of
 *     ten, up to 10^12, that divides them all, and keep its exponent in the
 *     scaler nibble; a one-row block has no delta to refuse 10^12 and
 *     carries 12 (timestamp.rs:97-121).
 *   f64  float.rs:32-243       [6][0x10][first f64 BE][bitstream]
 *     MSB-first; per further value 0 (repeat), 10 <bits> (XOR inside the
 *     previous window) or 11 <lead:5> <meaningful:6> <bits> (new window);
 *     the leading-zero count is cut to its low 5 bits before the window
 *     comparison, 64 meaningful bits are written as 0, GORILLA_SENTINEL is appended as the
 *     terminator and the last byte is zero-padded.  The sentinel as a later
 *     input value is an error (float.rs:58-60).
 *   bool boolean.rs:24-64      [10][0x10][varint n][bits MSB-first]
 *   page tsm/page.rs:488-497   [bitset_len u32 BE][nrows u64 BE][crc u32 BE]
 *                              [validity bitset, LSB-first][data block]
 *     crc: CRC-32/ISO-HDLC of the data block (page.rs:58-76).
 *
 * Plain integer code: no atomics, LDS or lane intrinsics, no allocation and
 * no std:: containers; errors are returned (TsmEncErr), never raised.  The
 * header also compiles as host C++ (tests/cpu/tsm_enc_check.cpp). */
#ifndef GS_TSM_ENC_H
#define GS_TSM_ENC_H

#include <cstddef>
#include <cstdint>
#include "../../include/cnosdb_gs.h"
#include "gs_internal.h"

#ifdef __HIPCC__ /* spelled out: gs_encode.cpp does not see hip_runtime.h */
#define TSM_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define TSM_FN inline
#endif

enum { TSM_SUB_UNCOMPRESSED = 0, TSM_SUB_SIMPLE8B = 1, TSM_SUB_RLE = 2 };

/* What an encoder returns instead of a length.  The device entry points
 * hand these to their callers as the failed page's length; the host entry
 * points map them to their own codes. */
enum TsmEncErr {
    TSM_ENC_ERR_SENTINEL = -1, /* GORILLA_SENTINEL as a non-first f64 value */
    TSM_ENC_ERR_RANGE = -2,    /* a value does not fit a simple8b word */
};

/* ------------------------------------------------------------ helpers */

TSM_FN void tsm_put_be32(uint8_t *p, uint32_t v) {
    for (int i = 3; i >= 0; i--) { p[i] = uint8_t(v); v >>= 8; }
}
TSM_FN void tsm_put_be64(uint8_t *p, uint64_t v) {
    for (int i = 7; i >= 0; i--) { p[i] = uint8_t(v); v >>= 8; }
}
TSM_FN uint64_t tsm_zigzag(int64_t v) {
    return (uint64_t(v) << 1) ^ uint64_t(v >> 63);
}
TSM_FN size_t tsm_varint_put(uint8_t *dst, uint64_t v) {
    size_t n = 0;
    while (v >= 0x80) { dst[n++] = uint8_t(v | 0x80); v >>= 7; }
    dst[n++] = uint8_t(v);
    return n;
}
TSM_FN size_t tsm_varint_len(uint64_t v) {
    size_t n = 1;
    while (v >= 0x80) { n++; v >>= 7; }
    return n;
}

/* ------------------------------------------------------------ simple8b */

/* {values per word, bits per value} of selector idx + 2 */
TSM_FN void tsm_s8b_shape(int idx, size_t &count, unsigned &bits) {
    constexpr uint8_t TSM_S8B[14][2] = {
        {60, 1}, {30, 2}, {20, 3}, {15, 4}, {12, 5}, {10, 6}, {8, 7},
        {7, 8},  {6, 10}, {5, 12}, {4, 15}, {3, 20}, {2, 30}, {1, 60},
    };
    count = TSM_S8B[idx][0];
    bits = TSM_S8B[idx][1];
}

/* Greedy packer over the values packed(0..m): a run of 240 or 120 ones
 * where at least that many values are left, else the first selector whose
 * word the next values fill.  8 bytes per word, never more than 8 * m. */
template <class Src>
TSM_FN int64_t tsm_s8b_pack(Src packed, size_t m, uint8_t *dst) {
    size_t i = 0, w = 0;
    while (i < m) {
        const size_t remain = m - i;
        if (remain >= 120) {
            const size_t lim = remain >= 240 ? 240 : 120;
            size_t k = 0;
            while (k < lim && packed(i + k) == 1) k++;
            if (k >= 120) {
                tsm_put_be64(dst + w, k == 240 ? 0 : 1ULL << 60);
                w += 8;
                i += k == 240 ? 240 : 120;
                continue;
            }
        }
        bool ok = false;
        for (int idx = 0; idx < 14; idx++) {
            size_t int_n;
            unsigned bit_n;
            tsm_s8b_shape(idx, int_n, bit_n);
            if (int_n > remain) continue;
            const uint64_t max_val = 1ULL << bit_n;
            uint64_t word = (uint64_t(idx) + 2) << 60;
            bool fits = true;
            for (size_t q = 0; q < int_n; q++) {
                const uint64_t pv = packed(i + q);
                if (pv >= max_val) { fits = false; break; }
                word |= pv << (unsigned(q) * bit_n);
            }
            if (!fits) continue;
            tsm_put_be64(dst + w, word);
            w += 8;
            i += int_n;
            ok = true;
            break;
        }
        if (!ok) return TSM_ENC_ERR_RANGE;
    }
    return int64_t(w);
}

/* ------------------------------------------------------------ ts / i64 */

/* The timestamp scaler: the largest power of ten up to 10^12 that divides
 * delta(1..n), and its exponent. */
template <class Delta>
TSM_FN uint64_t tsm_ts_scaler(Delta delta, size_t n, unsigned &exponent) {
    uint64_t div = 1000000000000ULL;
    for (size_t i = 1; i < n && div > 1; i++)
        while (div > 1 && delta(i) % div != 0) div /= 10;
    exponent = 0;
    for (uint64_t x = div; x > 1; x /= 10) exponent++;
    return div;
}

/* Worst case of a ts/i64 block: uncompressed, 8 bytes per value; the 16
 * cover the RLE block of a two-row page, whose varints can outgrow that.
 * gs_encode_ts/i64 ask for exactly this, the device entry points for 16
 * bytes more.  Which capacities are refused is part of each one's contract,
 * so the two thresholds stay apart. */
TSM_FN uint64_t tsm_int_max_len(uint64_t n) { return 2 + 8 * n + 16; }

/* Encodes the n values of src, all valid, as a ts (is_ts) or i64 block of
 * at most tsm_int_max_len(n) bytes; returns its length or
 * TSM_ENC_ERR_RANGE.  Multi-pass over src.  The simple8b path packs either
 * straight from src, recomputing a value each time the packer looks at it
 * (scratch == NULL: the device, one thread per page and no memory of its
 * own), or from scratch[0..n-1), filled once (the host, which then divides
 * by the scaler once per value). */
TSM_FN int64_t tsm_enc_int(bool is_ts, const int64_t *src, size_t n,
                           uint8_t *dst, uint64_t *scratch) {
    if (n == 0) return 0;
    auto delta = [&](size_t i) { /* i in 1..n */
        const uint64_t d = uint64_t(src[i]) - uint64_t(src[i - 1]);
        return is_ts ? d : tsm_zigzag(int64_t(d));
    };
    const uint64_t d0 = is_ts ? uint64_t(src[0]) : tsm_zigzag(src[0]);
    const uint64_t d1 = n > 1 ? delta(1) : 0;
    uint64_t max = 0;
    bool all_equal = true;
    for (size_t i = 1; i < n; i++) {
        const uint64_t d = delta(i);
        all_equal &= d == d1;
        if (d > max) max = d;
    }
    size_t w = 0;
    dst[w++] = is_ts ? GS_ENC_DELTATS : GS_ENC_DELTA;
    uint64_t div = 1;
    unsigned scaler = 0;
    if (all_equal && n > (is_ts ? 1u : 2u)) {
        if (is_ts) div = tsm_ts_scaler(delta, 2, scaler);
        dst[w++] = uint8_t((TSM_SUB_RLE << 4) | scaler);
        tsm_put_be64(dst + w, d0);
        w += 8;
        w += tsm_varint_put(dst + w, div > 1 ? d1 / div : d1);
        w += tsm_varint_put(dst + w, is_ts ? uint64_t(n) : uint64_t(n) - 1);
        return int64_t(w);
    }
    if (max > (1ULL << 60) - 1) {
        dst[w++] = uint8_t(TSM_SUB_UNCOMPRESSED << 4);
        tsm_put_be64(dst + w, d0);
        w += 8;
        for (size_t i = 1; i < n; i++) {
            tsm_put_be64(dst + w, delta(i));
            w += 8;
        }
        return int64_t(w);
    }
    if (is_ts) div = tsm_ts_scaler(delta, n, scaler);
    dst[w++] = uint8_t((TSM_SUB_SIMPLE8B << 4) | scaler);
    tsm_put_be64(dst + w, d0);
    w += 8;
    auto packed = [&](size_t j) { /* j in 0..n-1 */
        const uint64_t d = delta(j + 1);
        return div > 1 ? d / div : d;
    };
    int64_t s;
    if (scratch) {
        for (size_t j = 0; j + 1 < n; j++) scratch[j] = packed(j);
        s = tsm_s8b_pack([&](size_t j) { return scratch[j]; }, n - 1, dst + w);
    } else {
        s = tsm_s8b_pack(packed, n - 1, dst + w);
    }
    return s < 0 ? s : int64_t(w) + s;
}

/* ------------------------------------------------------------ Gorilla f64 */

/* Worst case of a Gorilla block over n non-null values: header, first
 * value, 10 bytes for each further value and the sentinel (at most 77
 * bits), 16 spare.  The capacity every f64 encode entry point asks for. */
TSM_FN uint64_t tsm_gorilla_max_len(uint64_t n) {
    return 2 + 8 + (n + 1) * 10 + 16;
}

/* MSB-first bit appender: bits gather at the top of acc and leave as whole
 * 8-byte words, so the output needs no zero fill */
struct TsmBitWriter {
    uint8_t *dst;
    size_t nbytes;
    uint64_t acc;
    unsigned nfill; /* bits in acc, < 64 between calls */
    TSM_FN void put(uint64_t x, unsigned l) { /* x < 2^l, 1 <= l <= 64 */
        if (nfill + l < 64) {
            acc |= x << (64 - nfill - l);
            nfill += l;
            return;
        }
        const unsigned rest = nfill + l - 64; /* bits of x that stay behind */
        tsm_put_be64(dst + nbytes, acc | (x >> rest));
        nbytes += 8;
        acc = rest ? x << (64 - rest) : 0;
        nfill = rest;
    }
    TSM_FN size_t finish() { /* zero-pads the last byte */
        for (; nfill > 0; nfill -= nfill < 8 ? nfill : 8) {
            dst[nbytes++] = uint8_t(acc >> 56);
            acc <<= 8;
        }
        return nbytes;
    }
};

/* Encodes the n values of v, all valid, as a Gorilla block of at most
 * tsm_gorilla_max_len(n) bytes; returns its length, 0 for n == 0, or
 * TSM_ENC_ERR_SENTINEL.  The first value is the header and is not checked
 * against the sentinel. */
TSM_FN int64_t tsm_enc_gorilla(const double *v, size_t n, uint8_t *dst) {
    auto bits = [&](size_t r) {
        uint64_t b;
        __builtin_memcpy(&b, v + r, 8);
        return b;
    };
    if (n == 0) return 0;
    size_t r = 0;
    dst[0] = GS_ENC_GORILLA;
    dst[1] = 1 << 4;
    uint64_t prev = bits(r++);
    tsm_put_be64(dst + 2, prev);
    TsmBitWriter bw = {dst + 10, 0, 0, 0};
    uint64_t prev_lead = ~0ULL, prev_trail = 0;
    for (;;) {
        uint64_t cur;
        if (r < n) {
            cur = bits(r++);
            if (cur == GORILLA_SENTINEL) return TSM_ENC_ERR_SENTINEL;
        } else {
            cur = GORILLA_SENTINEL;
        }
        const uint64_t x = cur ^ prev;
        if (x == 0) {
            bw.put(0, 1);
        } else {
            const uint64_t lead = uint64_t(__builtin_clzll(x)) & 0x1f;
            const uint64_t trail = uint64_t(__builtin_ctzll(x));
            if (prev_lead != ~0ULL && lead >= prev_lead && trail >= prev_trail) {
                bw.put(2, 2); /* 10 */
                bw.put(x >> prev_trail, unsigned(64 - prev_lead - prev_trail));
            } else {
                prev_lead = lead;
                prev_trail = trail;
                const uint64_t sig = 64 - lead - trail;
                /* 11, lead, meaningful (64 is written as 0) */
                bw.put((3u << 11) | (lead << 6) | (sig & 0x3f), 13);
                bw.put(x >> trail, unsigned(sig));
            }
        }
        prev = cur;
        if (cur == GORILLA_SENTINEL) break;
    }
    return int64_t(10 + bw.finish());
}

/* ------------------------------------------------------------ bool */

/* A bool block over n > 0 values is its header and then (n + 7) / 8 bytes
 * of tsm_bool_byte: tsm_bool_len(n) bytes exactly. */
TSM_FN size_t tsm_bool_header_len(uint64_t n) { return 2 + tsm_varint_len(n); }
TSM_FN size_t tsm_bool_len(uint64_t n) {
    return n ? tsm_bool_header_len(n) + size_t((n + 7) / 8) : 0;
}
TSM_FN size_t tsm_bool_header(uint8_t *dst, uint64_t n) {
    dst[0] = GS_ENC_BITPACK;
    dst[1] = 1 << 4;
    return 2 + tsm_varint_put(dst + 2, n);
}
/* byte j of the bit area: values src[8j .. 8j+8), first value highest */
TSM_FN uint8_t tsm_bool_byte(const uint8_t *src, size_t n, size_t j) {
    uint8_t byte = 0;
    for (int k = 0; k < 8; k++) {
        const size_t i = j * 8 + k;
        if (i < n && src[i]) byte |= uint8_t(0x80u >> k);
    }
    return byte;
}

/* ------------------------------------------------------------ page */

/* CRC-32/ISO-HDLC over a 256-entry table the caller keeps (a static on the
 * host, LDS in the kernels) */
TSM_FN uint32_t tsm_crc32_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    return c;
}
TSM_FN uint32_t tsm_crc32(const uint32_t *table, const uint8_t *data,
                          size_t len) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < len; i++) c = table[(c ^ data[i]) & 0xFF] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

/* the 16 bytes in front of a page's bitset */
TSM_FN void tsm_page_header(uint8_t *pg, uint32_t bitset_len, uint64_t nrows,
                            uint32_t crc) {
    tsm_put_be32(pg, bitset_len);
    tsm_put_be64(pg + 4, nrows);
    tsm_put_be32(pg + 12, crc);
}

#endif
