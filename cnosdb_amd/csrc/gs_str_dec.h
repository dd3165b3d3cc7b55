/* The string page decoder (codec/string.rs:169-309): the single home of
 * the snappy raw-stream decompressor, the payload walk and the scratch
 * slab accounting.  k_str_decode runs str_page_decode once per page and
 * gs_groups_upload sizes each page's slab with str_slab_size; the header
 * also compiles as host C++ (tests/cpu/str_decode_check.cpp), where the
 * same code runs under AddressSanitizer and UBSan on exact-size buffers.
 *
 * Page data:
 *   [7][0x10][snappy raw stream]   payload = varint length + bytes, per string
 *   [1][payload]                   payload = u64 BE length + bytes, per string
 *   (empty)                        every row null
 * Only valid rows consume a string; strings behind the last valid row are
 * ignored, as in the reference.
 *
 * Snappy raw stream: a varint preamble (the uncompressed length), then
 * elements tagged by the low two bits of their first byte:
 *   00  literal: length-1 in the tag's high 6 bits, or 60..63 = the
 *       length-1 follows in 1..4 little-endian bytes; then the bytes
 *   01  copy, 1-byte offset: length 4..11, offset 11 bits
 *   10  copy, 2-byte LE offset: length 1..64
 *   11  copy, 4-byte LE offset: length 1..64
 * A copy may overlap its own output (offset < length repeats a pattern).
 *
 * Every length, and every bound a length enters, is computed in 64 bits.
 * A stream element's length is at most 2^32 (a 4-byte literal field of
 * FF FF FF FF is 2^32 bytes, not 0), so its 64-bit address sums cannot
 * wrap; a string length in the payload can be anything up to 2^64-1 and is
 * compared against what is LEFT (slen > pn - i), never as cursor + length.
 *
 * Plain integer code, no atomics, LDS or lane intrinsics: raising errors
 * stays with the kernel. */
#ifndef GS_STR_DEC_H
#define GS_STR_DEC_H

#include <cstdint>

#ifdef __HIPCC__
#define STR_FN __host__ __device__ __forceinline__
#else
#define STR_FN inline
#endif

/* encoding byte of a string page (models/src/codec.rs:42-48) */
#define STR_ENC_NULL 1
#define STR_ENC_SNAPPY 7

/* str_page_decode verdicts; the values are the engine's DERR_* bits */
#define STR_OK 0u
#define STR_ERR_FORMAT 1u
#define STR_ERR_SHORT 2u

/* LEB128 u64 at p[0..n): bytes consumed (1..10), or 0 when the varint does
 * not end within n bytes or within 10. */
STR_FN uint32_t str_varint(const uint8_t *p, uint64_t n, uint64_t *out) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < n && i < 10; i++) {
        const uint8_t b = p[i];
        v |= uint64_t(b & 0x7f) << (7 * i);
        if (!(b & 0x80)) {
            *out = v;
            return i + 1;
        }
    }
    return 0;
}

/* What a page's payload can at most come to, from the page's length alone.
 * Snappy: the densest element is a 2-byte-offset copy, 64 bytes out of 3
 * stream bytes, so the output stays below 22 x the stream length (a literal
 * yields under 1 per byte, a 1-byte-offset copy 11 per 2, a 4-byte-offset
 * copy 64 per 5).  Null encoding: the payload as is. */
STR_FN uint64_t str_slab_bound(uint32_t data_len, uint8_t enc) {
    if (enc == STR_ENC_SNAPPY && data_len > 2)
        return 22 * (uint64_t(data_len) - 2);
    if (enc == STR_ENC_NULL && data_len >= 1) return uint64_t(data_len) - 1;
    return 0;
}

/* Bytes of scratch a page's payload gets: the snappy preamble, capped by
 * str_slab_bound.  A preamble above the bound cannot be honest and
 * str_snappy_decompress rejects it, against that same bound, before
 * writing; one within the bound gets exactly the slab it asks for. */
STR_FN uint64_t str_slab_size(const uint8_t *data, uint32_t data_len,
                              uint8_t enc) {
    const uint64_t bound = str_slab_bound(data_len, enc);
    if (enc != STR_ENC_SNAPPY || bound == 0) return bound;
    uint64_t ulen = 0;
    if (!str_varint(data + 2, uint64_t(data_len) - 2, &ulen)) return 0;
    return ulen < bound ? ulen : bound;
}

/* slabs start 16-byte aligned in the set's scratch */
STR_FN uint64_t str_slab_stride(uint64_t slab) {
    return (slab + 15) & ~uint64_t(15);
}

/* Decompress src[0..len) into dst, a slab of min(preamble, cap) bytes.
 * Returns the uncompressed length, or -1: unterminated preamble, preamble
 * above cap and so above the slab (returned before any byte is written), an element that runs off the stream or past the
 * preamble, a copy reaching before the output's start, offset 0, or an
 * output that ends short of the preamble. */
STR_FN int64_t str_snappy_decompress(const uint8_t *__restrict__ src,
                                     uint32_t len, uint8_t *__restrict__ dst,
                                     uint64_t cap) {
    uint64_t ulen = 0;
    const uint32_t hdr = str_varint(src, len, &ulen);
    if (!hdr || ulen > cap) return -1;
    const uint8_t *ip = src + hdr, *end = src + len;
    uint8_t *op = dst, *const op_end = dst + ulen; /* inside the slab */
    while (ip < end) {
        const uint8_t tag = *ip++;
        uint32_t l, off; /* of a copy: 1..64 bytes from up to 2^32-1 back */
        switch (tag & 3) {
        case 0: {
            uint64_t ll = tag >> 2; /* a literal is up to 2^32 bytes */
            if (ll >= 60) {
                const uint32_t c = uint32_t(ll) - 59;
                if (ip + c > end) return -1; /* c <= 4 */
                ll = 0;
                for (uint32_t k = 0; k < c; k++)
                    ll |= uint64_t(ip[k]) << (8 * k);
                ip += c;
            }
            ll += 1;
            /* 64-bit address sums: ll is at most 2^32, so neither wraps */
            if (ip + ll > end || op + ll > op_end) return -1;
            { /* word-wide literal copy (disjoint buffers; bounds above
                 guarantee the 8-B reads/writes stay inside [ip,ip+n) /
                 [op,op+n)).  The length fits 32 bits from here on: it is
                 at most the stream's. */
                const uint32_t n = uint32_t(ll);
                uint32_t k = 0;
                for (; k + 8 <= n; k += 8) {
                    uint64_t w;
                    __builtin_memcpy(&w, ip + k, 8);
                    __builtin_memcpy(op + k, &w, 8);
                }
                for (; k < n; k++) op[k] = ip[k];
                ip += n;
                op += n;
            }
            continue;
        }
        case 1:
            if (ip >= end) return -1;
            l = ((tag >> 2) & 7) + 4;
            off = (uint32_t(tag >> 5) << 8) | *ip++;
            break;
        case 2:
            if (ip + 2 > end) return -1;
            l = (tag >> 2) + 1;
            off = uint32_t(ip[0]) | (uint32_t(ip[1]) << 8);
            ip += 2;
            break;
        default:
            if (ip + 4 > end) return -1;
            l = (tag >> 2) + 1;
            off = uint32_t(ip[0]) | (uint32_t(ip[1]) << 8) |
                  (uint32_t(ip[2]) << 16) | (uint32_t(ip[3]) << 24);
            ip += 4;
            break;
        }
        /* op + l: at most 64 bytes past the slab's end, as an address */
        if (off == 0 || uint64_t(op - dst) < off || op + l > op_end) return -1;
        const uint8_t *cp = op - off; /* may overlap: strictly in order */
        if (off >= 8) { /* no overlap within a word: copy 8 B at a time */
            uint32_t k = 0;
            for (; k + 8 <= l; k += 8) {
                uint64_t w;
                __builtin_memcpy(&w, cp + k, 8);
                __builtin_memcpy(op + k, &w, 8);
            }
            for (; k < l; k++) op[k] = cp[k];
        } else { /* short offset: byte-serial repeat semantics */
            for (uint32_t k = 0; k < l; k++) op[k] = cp[k];
        }
        op += l;
    }
    return op == op_end ? int64_t(ulen) : -1;
}

STR_FN int str_bit(const uint8_t *bs, uint32_t r) {
    return (bs[r >> 3] >> (r & 7)) & 1;
}

/* Walk the payload pl[0..pn) against the validity bits: every valid row
 * takes the next length prefix (varint, or u64 BE when `be`) and records
 * pos[r] = pos_base + (index of its first byte), sz[r] = its length,
 * valid[r] = 1.  Rows not reached keep what the caller put there.  A
 * payload that is used up while valid rows remain is STR_ERR_SHORT (the
 * reference emits a shorter array there; failing loudly beats silently
 * nulling rows). */
STR_FN unsigned str_payload_walk(const uint8_t *__restrict__ pl, uint64_t pn,
                                 int be, const uint8_t *__restrict__ bs,
                                 int all_valid, uint32_t nrows,
                                 int64_t pos_base, int64_t *__restrict__ sz,
                                 int64_t *__restrict__ pos,
                                 uint8_t *__restrict__ valid) {
    uint64_t i = 0;
    for (uint32_t r = 0; r < nrows; r++) {
        if (!all_valid && !str_bit(bs, r)) continue;
        if (i >= pn) return STR_ERR_SHORT;
        uint64_t slen = 0;
        if (be) {
            if (pn - i < 8) return STR_ERR_FORMAT;
            for (int k = 0; k < 8; k++) slen = (slen << 8) | pl[i + k];
            i += 8;
        } else {
            slen = pl[i]; /* i < pn; most strings are under 128 bytes */
            if (slen < 0x80) {
                i += 1;
            } else {
                const uint32_t c = str_varint(pl + i, pn - i, &slen);
                if (!c) return STR_ERR_FORMAT;
                i += c;
            }
        }
        if (slen > pn - i) return STR_ERR_FORMAT;
        pos[r] = pos_base + int64_t(i);
        sz[r] = int64_t(slen);
        if (valid) valid[r] = 1;
        i += slen;
    }
    return STR_OK;
}

/* One page, start to end: clear its rows, bring the payload into the
 * page's slab (both encodings, so the walk and the later gather read one
 * source), walk it.  slab holds str_slab_size bytes of the same page and
 * slab_off is its offset in the set's scratch; sz / pos / valid point
 * at the page's first row.  Returns STR_OK or the STR_ERR_* to raise. */
STR_FN unsigned str_page_decode(const uint8_t *__restrict__ data,
                                uint32_t data_len, uint8_t enc,
                                const uint8_t *__restrict__ bs, int all_valid,
                                uint32_t nrows, uint8_t *__restrict__ slab,
                                int64_t slab_off,
                                int64_t *__restrict__ sz,
                                int64_t *__restrict__ pos,
                                uint8_t *__restrict__ valid) {
    for (uint32_t r = 0; r < nrows; r++) {
        sz[r] = 0;
        pos[r] = 0;
        if (valid) valid[r] = 0;
    }
    if (data_len == 0) return STR_OK; /* empty src -> all null,
                                         string.rs:231-236 */
    const uint64_t slab_cap = str_slab_bound(data_len, enc);
    uint64_t pn;
    int be = 0;
    if (enc == STR_ENC_SNAPPY) {
        if (data_len < 2) return STR_ERR_FORMAT;
        const int64_t n = str_snappy_decompress(data + 2, data_len - 2, slab,
                                                slab_cap);
        if (n < 0) return STR_ERR_FORMAT;
        pn = uint64_t(n);
    } else if (enc == STR_ENC_NULL) { /* string.rs:169-183 */
        pn = uint64_t(data_len) - 1;
        if (pn > slab_cap) return STR_ERR_FORMAT;
        for (uint64_t k = 0; k < pn; k++) slab[k] = data[1 + k];
        be = 1;
    } else {
        return STR_ERR_FORMAT;
    }
    return str_payload_walk(slab, pn, be, bs, all_valid, nrows, slab_off, sz,
                            pos, valid);
}

#endif
