/* The integer-family and bool page decoders: the single home of the
 * DeltaTs/Delta page header, the simple8b word rule, the BitPack header
 * and the page-sequential decodes.  The kernels of gs_engine.cpp and
 * gs_groups_upload go through it; the header also compiles as host C++
 * (tests/cpu/int_decode_check.cpp), where the same code runs under
 * AddressSanitizer and UBSan on exact-size buffers.
 *
 * Decode semantics mirror, bit-exactly:
 *   tskv/src/tsm/codec/timestamp.rs:177-299   (DeltaTs: sub-tag + scaler)
 *   tskv/src/tsm/codec/integer.rs:142-248     (Delta: zigzag)
 *   tskv/src/tsm/codec/simple8b.rs:80-208
 *   tskv/src/tsm/codec/boolean.rs:79-136
 *
 * Page data:
 *   [11|2][sub<<4 | scaler][...]    DeltaTs (time) / Delta (i64, u64)
 *      sub 0  uncompressed: BE64 deltas, the first one from 0
 *      sub 1  simple8b: first BE64, then BE64 words of packed deltas
 *      sub 2  RLE: first BE64, varint delta (the reference's repeat count
 *             behind it is not read: the page's row count rules)
 *      A time page stores its deltas as they are, divided by 10^scaler; an
 *      integer page zigzags the first value and every delta and has no
 *      scaler.
 *   [1][BE64 per valid row]         Null encoding, raw
 *   [10][0x10][varint n][bits]      BitPack bool, MSB first
 *   [1][byte per valid row]         Null encoding, bool
 *   (empty)                         every row null
 *
 * simple8b word: selector in the top 4 bits.  Selectors 0 and 1 are runs
 * of 240 and 120 ones without payload; selector s >= 2 holds count(s)
 * values of width(s) bits, lowest first.
 *
 * Plain integer code, no atomics, LDS or lane intrinsics: raising errors
 * stays with the kernels. */
#ifndef GS_INT_DEC_H
#define GS_INT_DEC_H

#include <cstdint>
#include "gs_str_dec.h" /* str_varint, the one LEB128 reader; str_bit */
#include "gs_tsm_enc.h" /* tsm_s8b_shape, the one selector table */

#ifdef __HIPCC__
#define INT_FN __host__ __device__ __forceinline__
#else
#define INT_FN inline
#endif

/* verdicts; the values are the engine's DERR_* bits */
#define INT_OK 0u
#define INT_ERR_FORMAT 1u
#define INT_ERR_SHORT 2u
#define INT_ERR_NONMONO 4u

INT_FN uint64_t int_be64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}
INT_FN int64_t int_zzdec(uint64_t v) {
    return int64_t((v >> 1) ^ uint64_t(-int64_t(v & 1)));
}

/* ---------------------------------------------------------------- simple8b */

/* Shape of one word: values it holds, bits per value (0: a run of ones)
 * and the mask of one value. */
INT_FN void int_s8b_word(uint64_t w, uint32_t &cnt, unsigned &bits,
                         uint64_t &mask) {
    const unsigned sel = unsigned(w >> 60);
    if (sel <= 1) {
        cnt = sel ? 120 : 240;
        bits = 0;
    } else {
        size_t c;
        tsm_s8b_shape(int(sel) - 2, c, bits);
        cnt = uint32_t(c);
    }
    mask = (1ULL << bits) - 1; /* bits <= 60 */
}
/* value k of a word of that shape */
INT_FN uint64_t int_s8b_get(uint64_t w, uint32_t k, unsigned bits,
                            uint64_t mask) {
    return bits ? (w >> (k * bits)) & mask : 1;
}

/* word stream, one value per call (simple8b.rs:95-208) */
struct IntS8b {
    const uint8_t *p;
    uint32_t len, pos;
    uint64_t word, mask;
    uint32_t idx, cnt;
    unsigned bits;
    INT_FN void init(const uint8_t *p_, uint32_t len_) {
        p = p_; len = len_; pos = 0; idx = 0; cnt = 0; bits = 0; word = 0;
        mask = 0;
    }
    INT_FN bool next(uint64_t *out) {
        if (idx >= cnt) {
            if (pos + 8 > len) return false;
            word = int_be64(p + pos);
            pos += 8;
            int_s8b_word(word, cnt, bits, mask);
            idx = 0;
        }
        *out = int_s8b_get(word, idx++, bits, mask);
        return true;
    }
};

/* ------------------------------------------------- DeltaTs / Delta header */

struct IntHeader {
    unsigned verdict;  /* INT_OK, or the INT_ERR_* to raise; first, rle_delta
                          and the payload are 0 then */
    bool is_ts;        /* DeltaTs: plain deltas x scaler; else zigzag */
    unsigned sub;      /* TSM_SUB_*; 0 unless a DeltaTs/Delta page has one */
    uint64_t scaler;   /* 10^(low nibble) of a time page, else 1 */
    int64_t first;     /* sub 1, 2: the first value */
    int64_t rle_delta; /* sub 2: the step, scaled / unzigzagged */
    const uint8_t *payload; /* sub 0: the deltas; sub 1: the words */
    uint32_t payload_len;
};

/* The only reader of the sub-tag byte, the scaler nibble, the first value
 * and the RLE varint.  enc is data[0]. */
INT_FN IntHeader int_page_header(const uint8_t *data, uint32_t data_len,
                                 uint8_t enc) {
    IntHeader h = {INT_ERR_FORMAT, enc == GS_ENC_DELTATS, 0, 1, 0, 0,
                   nullptr, 0};
    if ((!h.is_ts && enc != GS_ENC_DELTA) || data_len < 2) return h;
    h.sub = data[1] >> 4;
    if (h.is_ts)
        for (unsigned k = data[1] & 15; k; k--) h.scaler *= 10;
    const uint8_t *q = data + 2;
    const uint32_t plen = data_len - 2;
    if (h.sub == TSM_SUB_UNCOMPRESSED) {
        if (plen == 0 || (plen & 7)) return h;
        h.payload = q;
        h.payload_len = plen;
    } else if (h.sub == TSM_SUB_RLE) {
        uint64_t dv;
        if (plen < 9 || !str_varint(q + 8, plen - 8, &dv)) return h;
        h.rle_delta = h.is_ts ? int64_t(dv * h.scaler) : int_zzdec(dv);
    } else if (h.sub == TSM_SUB_SIMPLE8B) {
        if (plen < 8) { h.verdict = INT_ERR_SHORT; return h; }
        h.payload = q + 8;
        h.payload_len = plen - 8;
    } else {
        return h;
    }
    if (h.sub != TSM_SUB_UNCOMPRESSED)
        h.first = h.is_ts ? int64_t(int_be64(q)) : int_zzdec(int_be64(q));
    h.verdict = INT_OK;
    return h;
}

/* a time RLE page that runs backwards */
INT_FN unsigned int_rle_nonmono(const IntHeader &h, uint32_t nrows) {
    return h.is_ts && h.rle_delta < 0 && nrows > 1 ? INT_ERR_NONMONO : INT_OK;
}

/* One int64-family page (TIME/I64/U64), row by row through the validity
 * bits: DeltaTs/Delta with all three sub-tags plus Null (raw BE), null
 * rows 0.  o / vd point at the page's first row; vd may be null.  time_col
 * holds a Null-encoded page to ascending values, as the delta forms are by
 * is_ts.  Returns the INT_ERR_* bits to raise. */
INT_FN unsigned int_page_decode(const uint8_t *__restrict__ data,
                                uint32_t data_len, uint8_t enc, bool time_col,
                                const uint8_t *__restrict__ bs, int all_valid,
                                uint32_t n, int64_t *__restrict__ o,
                                uint8_t *__restrict__ vd) {
    unsigned e = INT_OK;
    if (data_len == 0) { /* all-null (timestamp.rs:181-185) */
        for (uint32_t r = 0; r < n; r++) { o[r] = 0; if (vd) vd[r] = 0; }
        return e;
    }
    if (enc == GS_ENC_NULL) { /* raw BE per valid slot */
        const uint8_t *q = data + 1;
        uint32_t avail = (data_len - 1) / 8, used = 0;
        int64_t prev_ts = INT64_MIN;
        for (uint32_t r = 0; r < n; r++) {
            int v = all_valid ? 1 : str_bit(bs, r);
            if (v && used < avail) {
                int64_t x = int64_t(int_be64(q + 8ull * used)); used++;
                if (time_col) {
                    if (x < prev_ts) e |= INT_ERR_NONMONO;
                    prev_ts = x;
                }
                o[r] = x;
            }
            else { o[r] = 0; v = 0; }
            if (vd) vd[r] = uint8_t(v);
        }
        return e;
    }
    const IntHeader h = int_page_header(data, data_len, enc);
    if (h.verdict) return h.verdict;
    const bool is_ts = h.is_ts;

    if (h.sub == TSM_SUB_UNCOMPRESSED) {
        uint32_t avail = h.payload_len / 8, used = 0;
        int64_t prev = 0;
        for (uint32_t r = 0; r < n; r++) {
            int v = all_valid ? 1 : str_bit(bs, r);
            if (!v) { o[r] = 0; if (vd) vd[r] = 0; continue; }
            if (used >= avail) { /* ts silently stops (timestamp.rs:216) */
                if (!is_ts) e |= INT_ERR_SHORT;
                o[r] = 0; if (vd) vd[r] = uint8_t(is_ts ? 1 : 0);
                continue;
            }
            uint64_t raw = int_be64(h.payload + 8ull * used);
            used++;
            int64_t nxt = is_ts ? int64_t(uint64_t(prev) + raw)
                                : int64_t(uint64_t(prev) +
                                          uint64_t(int_zzdec(raw)));
            if (is_ts && nxt < prev && used > 1) e |= INT_ERR_NONMONO;
            prev = nxt;
            o[r] = prev;
            if (vd) vd[r] = 1;
        }
        return e;
    }
    if (h.sub == TSM_SUB_RLE) {
        e |= int_rle_nonmono(h, n);
        int64_t cur = h.first;
        bool first = true;
        for (uint32_t r = 0; r < n; r++) {
            int v = all_valid ? 1 : str_bit(bs, r);
            if (!v) { o[r] = 0; if (vd) vd[r] = 0; continue; }
            if (first) { o[r] = cur; first = false; }
            else { cur = int64_t(uint64_t(cur) + uint64_t(h.rle_delta)); o[r] = cur; }
            if (vd) vd[r] = 1;
        }
        return e;
    }
    /* simple8b */
    int64_t cur = h.first;
    IntS8b it;
    it.init(h.payload, h.payload_len);
    bool first = true;
    for (uint32_t r = 0; r < n; r++) {
        int v = all_valid ? 1 : str_bit(bs, r);
        if (!v) { o[r] = 0; if (vd) vd[r] = 0; continue; }
        if (first) { o[r] = cur; first = false; if (vd) vd[r] = 1; continue; }
        uint64_t u;
        if (!it.next(&u)) { o[r] = 0; if (vd) vd[r] = 1; continue; } /* iterator exhaustion: builder skips */
        int64_t nxt = is_ts ? int64_t(uint64_t(cur) + u * h.scaler)
                            : int64_t(uint64_t(cur) + uint64_t(int_zzdec(u)));
        if (is_ts && nxt < cur) e |= INT_ERR_NONMONO;
        cur = nxt;
        o[r] = cur;
        if (vd) vd[r] = 1;
    }
    return e;
}

/* ------------------------------------------------------------ BitPack bool */

struct BoolHeader {
    unsigned verdict;    /* INT_OK or INT_ERR_FORMAT */
    const uint8_t *bits; /* MSB first */
    uint64_t count;      /* declared, capped at the bits the page holds */
};

/* [10][0x10][varint count][bits].  The count is capped at 8 x the bytes
 * behind the varint, so `row's bit index >= count` is the one test for a
 * bit the page does not carry (the reference panics on the slice index
 * there, boolean.rs:100). */
INT_FN BoolHeader bool_page_header(const uint8_t *data, uint32_t data_len,
                                   uint8_t enc) {
    BoolHeader h = {INT_ERR_FORMAT, nullptr, 0};
    if (enc != GS_ENC_BITPACK || data_len < 2 || data[1] != (1 << 4)) return h;
    const uint32_t nr = str_varint(data + 2, data_len - 2, &h.count);
    if (!nr) return h;
    h.bits = data + 2 + nr;
    const uint64_t have = 8 * uint64_t(data_len - 2 - nr);
    if (h.count > have) h.count = have;
    h.verdict = INT_OK;
    return h;
}
INT_FN uint8_t bool_bit(const uint8_t *bits, uint64_t i) {
    return (bits[i >> 3] >> (7 - (i & 7))) & 1;
}

/* One bool page, row by row through the validity bits; as int_page_decode. */
INT_FN unsigned bool_page_decode(const uint8_t *__restrict__ data,
                                 uint32_t data_len, uint8_t enc,
                                 const uint8_t *__restrict__ bs, int all_valid,
                                 uint32_t n, uint8_t *__restrict__ o,
                                 uint8_t *__restrict__ vd) {
    if (data_len == 0) {
        for (uint32_t r = 0; r < n; r++) { o[r] = 0; if (vd) vd[r] = 0; }
        return INT_OK;
    }
    if (enc == GS_ENC_NULL) { /* boolean.rs:111-136 */
        const uint8_t *q = data + 1;
        uint32_t avail = data_len - 1, used = 0;
        for (uint32_t r = 0; r < n; r++) {
            int v = all_valid ? 1 : str_bit(bs, r);
            if (v && used < avail) { o[r] = (q[used] == 1); used++; }
            else { o[r] = 0; v = 0; }
            if (vd) vd[r] = uint8_t(v);
        }
        return INT_OK;
    }
    const BoolHeader h = bool_page_header(data, data_len, enc);
    if (h.verdict) return h.verdict;
    unsigned e = INT_OK;
    uint64_t bi = 0;
    for (uint32_t r = 0; r < n; r++) {
        int v = all_valid ? 1 : str_bit(bs, r);
        if (!v) { o[r] = 0; if (vd) vd[r] = 0; continue; }
        if (bi >= h.count) { e |= INT_ERR_SHORT; o[r] = 0; if (vd) vd[r] = 0; continue; }
        o[r] = bool_bit(h.bits, bi);
        bi++;
        if (vd) vd[r] = 1;
    }
    return e;
}

#endif
