/* The string block encoder (codec/string.rs:32-88): the single home of the
 * payload framing and of the snappy raw-stream compressor.  gs_encode_str
 * (gs_encode.cpp) and the device kernel k_str_enc_pages (gs_engine.cpp) both
 * go through the functions below, so a string block encoded on the host and
 * one encoded on the device are the same code's output; the header also
 * compiles as host C++ (tests/cpu/str_enc_check.cpp), where the device's
 * loads run under AddressSanitizer and UBSan on exact-size buffers.
 *
 * Block:    [7 = Encoding::Snappy][0x10 = STRING_COMPRESSED_SNAPPY << 4]
 *           [varint payload length][one snappy fragment per 64 KiB of payload]
 * Payload:  [LEB128 varint len][bytes] per string, non-null strings only.
 * No strings at all is an empty block (0 bytes), not an empty payload.
 *
 * The compressor restates the published reference algorithm used by the
 * un-vendored `snap` crate v1.1.1 (64 KiB fragments, power-of-two hash table
 * in [256,16384] of 4-byte little-endian loads hashed by *0x1e35a7bd>>shift,
 * skip-32 acceleration, 15-byte tail margin); its output is pinned
 * byte-exactly by the reference's own golden vectors (string.rs:529-566),
 * checked in tests/test_encoders.py.  Independent of oracle/tsm_oracle.c.
 * It emits literals with 0, 1 or 2 length bytes and copies with 1- or
 * 2-byte offsets only: a fragment is at most 65536 bytes.
 *
 * Reading the four bytes at p is the one place where host and device
 * differ: the host keeps its memcpy, the device (and a host build with
 * STR_ENC_BYTE_LOADS) shifts the word out of the one or two aligned words
 * around p and copies literals byte by byte, because p has any alignment
 * (see the hazard note in DESIGN.md; four single-byte loads were put back
 * together into one unaligned load by the compiler).  The payload buffer
 * must therefore start on a 4-byte boundary or be preceded by up to 3
 * readable bytes.
 *
 * Plain integer code: no atomics, LDS or lane intrinsics, no allocation and
 * no std:: containers.  The caller passes the hash table (uint16_t
 * [str_enc_table_size(min(payload, 65536))], at most 16384 entries) and the
 * payload buffer. */
#ifndef GS_STR_ENC_H
#define GS_STR_ENC_H

#include <cstddef>
#include <cstdint>
#include "gs_tsm_enc.h" /* tsm_varint_put, tsm_varint_len */

#if defined(__HIP_DEVICE_COMPILE__) || defined(STR_ENC_BYTE_LOADS)
#define STR_ENC_BYTEWISE 1
#else
#define STR_ENC_BYTEWISE 0
#endif

#define STR_ENC_FRAGMENT 65536u
#define STR_ENC_MAX_TABLE 16384u

/* Worst case of a string block over `payload` payload bytes: the two header
 * bytes, 32 for the preamble and slack, and snappy's own bound of one tag
 * byte per 6 literal bytes.  The capacity every string encode entry point
 * asks for. */
TSM_FN uint64_t str_enc_max_len(uint64_t payload) {
    return 2 + 32 + payload + payload / 6;
}

/* bytes of payload the n strings of `lens` come to */
TSM_FN uint64_t str_enc_payload_len(const uint64_t *lens, int64_t n) {
    uint64_t payload = 0;
    for (int64_t i = 0; i < n; i++) payload += lens[i] + tsm_varint_len(lens[i]);
    return payload;
}

TSM_FN uint32_t str_enc_load32(const uint8_t *p) {
#if STR_ENC_BYTEWISE
    /* the one or two aligned words that hold p[0..4): nothing below
       p & ~3 and nothing from p + 7 on is touched, and every p the
       compressor loads from is at least 15 bytes in front of its
       fragment's end */
    const uintptr_t a = uintptr_t(p);
    const uint8_t *w = p - (a & 3);
    const unsigned sh = unsigned(a & 3) * 8;
    uint32_t lo, hi;
    __builtin_memcpy(&lo, __builtin_assume_aligned(w, 4), 4);
    if (sh == 0) return lo;
    __builtin_memcpy(&hi, __builtin_assume_aligned(w + 4, 4), 4);
    return lo >> sh | hi << (32 - sh);
#else
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
#endif
}

TSM_FN void str_enc_copy(uint8_t *dst, const uint8_t *src, size_t n) {
#if STR_ENC_BYTEWISE
#pragma clang loop vectorize(disable) interleave(disable)
    for (size_t i = 0; i < n; i++) dst[i] = src[i];
#else
    __builtin_memcpy(dst, src, n);
#endif
}

/* the payload of n strings lying back to back in src */
TSM_FN void str_enc_payload(const uint8_t *src, const uint64_t *lens, int64_t n,
                            uint8_t *buf) {
    size_t p = 0, s = 0;
    for (int64_t i = 0; i < n; i++) {
        p += tsm_varint_put(buf + p, lens[i]);
        str_enc_copy(buf + p, src + s, size_t(lens[i]));
        p += size_t(lens[i]);
        s += size_t(lens[i]);
    }
}

/* a literal of n >= 1 bytes */
TSM_FN uint8_t *str_enc_lit(uint8_t *op, const uint8_t *p, size_t n) {
    if (n - 1 < 60) {
        *op++ = uint8_t((n - 1) << 2);
    } else {
        uint8_t *tag = op++;
        size_t v = n - 1;
        int nb = 0;
        for (; v; v >>= 8) *op++ = uint8_t(v), nb++;
        *tag = uint8_t((59 + nb) << 2);
    }
    str_enc_copy(op, p, n);
    return op + n;
}

/* one copy element, 4 <= len <= 64 */
TSM_FN uint8_t *str_enc_copy1(uint8_t *op, size_t off, size_t len) {
    if (len < 12 && off < 2048) {
        *op++ = uint8_t(1 | ((len - 4) << 2) | ((off >> 8) << 5));
        *op++ = uint8_t(off);
    } else {
        *op++ = uint8_t(2 | ((len - 1) << 2));
        *op++ = uint8_t(off);
        *op++ = uint8_t(off >> 8);
    }
    return op;
}

/* a match of any length, split so that no piece is shorter than 4 */
TSM_FN uint8_t *str_enc_copy_any(uint8_t *op, size_t off, size_t len) {
    for (; len >= 68; len -= 64) op = str_enc_copy1(op, off, 64);
    if (len > 64) op = str_enc_copy1(op, off, 60), len -= 60;
    return str_enc_copy1(op, off, len);
}

/* entries of the hash table a fragment of n bytes uses */
TSM_FN uint32_t str_enc_table_size(size_t n) {
    uint32_t tsz = 256;
    while (tsz < STR_ENC_MAX_TABLE && tsz < n) tsz <<= 1;
    return tsz;
}

/* Compresses the fragment in[0..n), 1 <= n <= 65536, to op and returns the
 * end of what it wrote.  tab[0..str_enc_table_size(n)) must be zero. */
TSM_FN uint8_t *str_enc_fragment(const uint8_t *in, size_t n, uint8_t *op,
                                 uint16_t *tab) {
    const int shift = 32 - __builtin_ctz(str_enc_table_size(n));
    const uint8_t *ip = in, *iend = in + n, *nmit = in;
    if (n >= 15) {
        const uint8_t *ilim = iend - 15;
        uint32_t nh = (str_enc_load32(++ip) * 0x1e35a7bdu) >> shift;
        for (;;) {
            uint32_t skip = 32;
            const uint8_t *nip = ip, *cand;
            do {
                ip = nip;
                uint32_t h = nh, adv = skip >> 5;
                skip += adv;
                nip = ip + adv;
                if (nip > ilim) goto tail;
                nh = (str_enc_load32(nip) * 0x1e35a7bdu) >> shift;
                cand = in + tab[h];
                tab[h] = uint16_t(ip - in);
            } while (str_enc_load32(ip) != str_enc_load32(cand));
            op = str_enc_lit(op, nmit, size_t(ip - nmit));
            uint32_t c32;
            do {
                const uint8_t *b = ip;
                const uint8_t *m1 = cand + 4, *m2 = ip + 4;
                while (m2 < iend && *m1 == *m2) m1++, m2++;
                size_t mlen = size_t(m2 - ip);
                ip += mlen;
                op = str_enc_copy_any(op, size_t(b - cand), mlen);
                nmit = ip;
                if (ip >= ilim) goto tail;
                uint32_t hp = (str_enc_load32(ip - 1) * 0x1e35a7bdu) >> shift;
                tab[hp] = uint16_t(ip - 1 - in);
                uint32_t hc = (str_enc_load32(ip) * 0x1e35a7bdu) >> shift;
                cand = in + tab[hc];
                c32 = str_enc_load32(cand);
                tab[hc] = uint16_t(ip - in);
            } while (str_enc_load32(ip) == c32);
            nh = (str_enc_load32(++ip) * 0x1e35a7bdu) >> shift;
        }
    }
tail:
    if (nmit < iend) op = str_enc_lit(op, nmit, size_t(iend - nmit));
    return op;
}

/* what stands in front of the fragments; payload >= 1 */
TSM_FN size_t str_enc_block_header(uint8_t *dst, uint64_t payload) {
    dst[0] = 7;    /* Encoding::Snappy */
    dst[1] = 0x10; /* STRING_COMPRESSED_SNAPPY << 4 */
    return 2 + tsm_varint_put(dst + 2, payload);
}

/* The whole block over buf[0..payload), payload >= 1, one fragment after
 * another: at most str_enc_max_len(payload) bytes at dst; returns the
 * length.  The serial form: the device kernel runs the same steps with the
 * table zeroed by its whole wave. */
TSM_FN int64_t str_enc_block(const uint8_t *buf, uint64_t payload, uint8_t *dst,
                             uint16_t *tab) {
    uint8_t *op = dst + str_enc_block_header(dst, payload);
    for (uint64_t off = 0; off < payload; off += STR_ENC_FRAGMENT) {
        const size_t frag = payload - off < STR_ENC_FRAGMENT
                                ? size_t(payload - off) : STR_ENC_FRAGMENT;
        const uint32_t tsz = str_enc_table_size(frag);
        for (uint32_t i = 0; i < tsz; i++) tab[i] = 0;
        op = str_enc_fragment(buf + off, frag, op, tab);
    }
    return int64_t(op - dst);
}

#endif
