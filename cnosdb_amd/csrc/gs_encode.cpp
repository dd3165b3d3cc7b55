/* Host-side write path of the cnosdb_gs engine: the C entry points of the
 * TSM DataBlock encoders and of page assembly (the reference's
 * Page::arrow_array_to_page, tsm/page.rs:100-353,488-497), plus the string
 * block encoder.  The ts/i64/f64/bool codecs, the CRC and the page header
 * are the functions of gs_tsm_enc.h, the string block those of
 * gs_str_enc.h, the same ones the device kernels run;
 * this file checks capacities and maps their errors to the public codes.
 * Used by the GPU read path's fixture/flush side; runs on host CPU exactly
 * as the reference writer does.  Bytes of dst behind the returned length
 * are unspecified.
 */
#include "gs_str_enc.h"
#include "gs_tsm_enc.h"
#include <cstring>
#include <memory>

namespace {

/* TsmEncErr -> what gs_encode_* have always returned */
int64_t host_code(int64_t r) {
    if (r == TSM_ENC_ERR_SENTINEL) return GS_ERR_SENTINEL;
    if (r == TSM_ENC_ERR_RANGE) return -1; /* value out of simple8b range */
    return r;
}

int64_t encode_int(bool is_ts, const int64_t *src, size_t n, uint8_t *dst,
                   size_t cap) {
    if (n == 0) return 0;
    if (cap < tsm_int_max_len(n)) return GS_ERR_CAP;
    /* the packed values once, for the packer to look at more than once */
    std::unique_ptr<uint64_t[]> scratch(new uint64_t[n]);
    return host_code(tsm_enc_int(is_ts, src, n, dst, scratch.get()));
}

} // namespace

extern "C" {

int64_t gs_encode_ts(const int64_t *src, size_t n, uint8_t *dst, size_t cap) {
    return encode_int(true, src, n, dst, cap);
}

int64_t gs_encode_i64(const int64_t *src, size_t n, uint8_t *dst, size_t cap) {
    return encode_int(false, src, n, dst, cap);
}

int64_t gs_encode_f64(const double *src, size_t n, uint8_t *dst, size_t cap) {
    if (n == 0) return 0;
    if (cap < tsm_gorilla_max_len(n)) return GS_ERR_CAP;
    return host_code(tsm_enc_gorilla(src, n, dst));
}

int64_t gs_encode_bool(const uint8_t *src, size_t n, uint8_t *dst, size_t cap) {
    if (n == 0) return 0;
    const size_t nb = (n + 7) / 8;
    if (cap < 1 + 8 + nb + 2) return GS_ERR_CAP;
    uint8_t *bits = dst + tsm_bool_header(dst, n);
    for (size_t j = 0; j < nb; j++) bits[j] = tsm_bool_byte(src, n, j);
    return int64_t(bits + nb - dst);
}

uint32_t gs_crc32(const uint8_t *data, size_t len) {
    static const struct Table {
        uint32_t t[256];
        Table() { for (uint32_t i = 0; i < 256; i++) t[i] = tsm_crc32_entry(i); }
    } table;
    return tsm_crc32(table.t, data, len);
}

/* string block encoder (codec/string.rs:32-88): the framing and the snappy
 * compressor are gs_str_enc.h, the source the device kernel runs too */
int64_t gs_encode_str(const uint8_t *src, const uint64_t *lens, int64_t nstr,
                      uint8_t *dst, size_t cap) {
    if (nstr == 0) return 0;
    const uint64_t payload = str_enc_payload_len(lens, nstr);
    if (cap < str_enc_max_len(payload)) return -5;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[payload]);
    std::unique_ptr<uint16_t[]> tab(new uint16_t[STR_ENC_MAX_TABLE]);
    str_enc_payload(src, lens, nstr, buf.get());
    return str_enc_block(buf.get(), payload, dst, tab.get());
}

/* page assembly, tsm/page.rs:488-497 */
int64_t gs_build_page(const uint8_t *bitset, int64_t nrows, const uint8_t *data,
                      size_t data_len, uint8_t *dst, size_t cap) {
    size_t bl = size_t((nrows + 7) / 8);
    size_t total = 16 + bl + data_len;
    if (cap < total) return -5;
    tsm_page_header(dst, uint32_t(bl), uint64_t(nrows),
                    gs_crc32(data, data_len));
    memcpy(dst + 16, bitset, bl);
    memcpy(dst + 16 + bl, data, data_len);
    return int64_t(total);
}

/* OpenMP batch Gorilla encode: one page per chunk of `rows_per_page`
 * consecutive values (fixture/flush helper; mirrors the writer loop of
 * TsmWriter::write_record_batch, tsm/writer.rs:249-314). Each page is
 * written at dst + p*cap_per_page; returns 0 and fills out_lens. */
int32_t gs_encode_f64_pages_omp(const double *vals, int64_t rows_per_page,
                                int64_t npages, uint8_t *dst,
                                int64_t cap_per_page, int64_t *out_lens,
                                int32_t nthreads) {
    (void)nthreads; /* used only via the OMP clause below */
    int32_t err = 0;
#pragma omp parallel for schedule(dynamic, 1) num_threads(nthreads)
    for (int64_t p = 0; p < npages; p++) {
        int64_t n = gs_encode_f64(vals + p * rows_per_page, size_t(rows_per_page),
                                  dst + p * cap_per_page, size_t(cap_per_page));
        out_lens[p] = n;
        if (n < 0) {
#pragma omp atomic write
            err = int32_t(n);
        }
    }
    return err;
}

const char *gs_version(void) { return "cnosdb_gs 0.1 (gfx950)"; }

} // extern "C"
