/* Host check of the write-side codecs (cnosdb_amd/csrc/gs_tsm_enc.h), the
 * code the device kernels run, built with AddressSanitizer and UBSan by
 * tests/test_tsm_enc_cpu.py.
 *
 * Input file (little-endian), written by the test:
 *   u32 ncases
 *   per case: u32 kind (0 ts, 1 i64, 2 f64, 3 bool), u32 nrows,
 *             u32 has_valid, i32 expect (block length, or a TsmEncErr),
 *             u32 crc of the expected block, 16 bytes expected page header,
 *             the values (8 bytes per row; bool 1 byte per row),
 *             nrows validity bytes if has_valid (f64 only),
 *             the expected block (expect bytes, if positive)
 *
 * Every case is encoded into a heap block of exactly the documented worst
 * case (tsm_int_max_len, tsm_gorilla_max_len of the non-null count,
 * tsm_bool_len), so a write past it is an ASan error; the inputs and the
 * packer's scratch sit in exact heap blocks as well.  An f64 case with
 * validity bytes is first gathered into an exact block of its non-null
 * values, in row order: what k_enc_prepare hands the encoder on the
 * device.  Length and bytes are
 * compared, then the block's CRC and the page header written from it.
 * ts/i64 cases run twice: packing straight from the column, as the device
 * does, and from the scratch array, as the host does. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "gs_tsm_enc.h"

enum { K_TS = 0, K_I64 = 1, K_F64 = 2, K_BOOL = 3 };

struct Case {
    uint32_t kind, nrows, has_valid, crc;
    int32_t expect;
    uint8_t header[16];
    std::unique_ptr<uint8_t[]> vals, valid, block;
};

static uint32_t crc_table[256];

static bool read_exact(FILE *f, void *dst, size_t n) {
    return n == 0 || fread(dst, 1, n, f) == n;
}

static size_t nonnull(const Case &c) {
    size_t nn = 0;
    for (uint32_t r = 0; r < c.nrows; r++) nn += !c.valid || c.valid[r];
    return nn;
}

/* one encode of a case; int_scratch picks the int encoder's source */
static int64_t encode(const Case &c, bool int_scratch, uint8_t *out) {
    const size_t n = c.nrows;
    if (c.kind == K_F64) {
        const double *v = (const double *)c.vals.get();
        if (!c.valid) return tsm_enc_gorilla(v, n, out);
        const size_t nn = nonnull(c);
        std::unique_ptr<double[]> dense(new double[nn]);
        for (size_t r = 0, k = 0; r < n; r++)
            if (c.valid[r]) __builtin_memcpy(&dense[k++], v + r, 8);
        return tsm_enc_gorilla(dense.get(), nn, out);
    }
    if (c.kind == K_BOOL) {
        if (n == 0) return 0;
        /* the host's loop; k_enc_prepare gives one j to a thread */
        uint8_t *bits = out + tsm_bool_header(out, n);
        if (size_t(bits - out) != tsm_bool_header_len(n)) return -100;
        for (size_t j = 0; j < (n + 7) / 8; j++)
            bits[j] = tsm_bool_byte(c.vals.get(), n, j);
        return int64_t(tsm_bool_len(n));
    }
    std::unique_ptr<uint64_t[]> scratch;
    if (int_scratch) scratch.reset(new uint64_t[n ? n - 1 : 0]);
    return tsm_enc_int(c.kind == K_TS, (const int64_t *)c.vals.get(), n, out,
                       int_scratch ? scratch.get() : nullptr);
}

static size_t worst_case(const Case &c) {
    if (c.kind == K_BOOL) return tsm_bool_len(c.nrows);
    if (c.kind != K_F64) return size_t(tsm_int_max_len(c.nrows));
    return size_t(tsm_gorilla_max_len(nonnull(c)));
}

static int check(const Case &c, int ci, bool int_scratch) {
    const size_t cap = worst_case(c);
    std::unique_ptr<uint8_t[]> out(new uint8_t[cap]);
    memset(out.get(), 0xA5, cap);
    const int64_t got = encode(c, int_scratch, out.get());
    const char *how = int_scratch ? "scratch" : "direct";
    if (got != c.expect) {
        printf("case %d (%s): length %lld != %d\n", ci, how, (long long)got,
               c.expect);
        return 1;
    }
    if (got < 0) return 0;
    if (memcmp(out.get(), c.block.get(), size_t(got)) != 0) {
        printf("case %d (%s): bytes differ\n", ci, how);
        return 1;
    }
    if (tsm_crc32(crc_table, out.get(), size_t(got)) != c.crc) {
        printf("case %d (%s): crc differs\n", ci, how);
        return 1;
    }
    std::unique_ptr<uint8_t[]> hdr(new uint8_t[16]);
    tsm_page_header(hdr.get(), (c.nrows + 7) / 8, c.nrows,
                    tsm_crc32(crc_table, out.get(), size_t(got)));
    if (memcmp(hdr.get(), c.header, 16) != 0) {
        printf("case %d (%s): page header differs\n", ci, how);
        return 1;
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    for (uint32_t i = 0; i < 256; i++) crc_table[i] = tsm_crc32_entry(i);
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4)) return 2;
    int bad = 0, nenc = 0;
    for (uint32_t ci = 0; ci < ncases; ci++) {
        Case c;
        uint32_t hdr[5];
        if (!read_exact(f, hdr, sizeof(hdr)) || !read_exact(f, c.header, 16))
            return 2;
        c.kind = hdr[0];
        c.nrows = hdr[1];
        c.has_valid = hdr[2];
        c.expect = int32_t(hdr[3]);
        c.crc = hdr[4];
        const size_t vbytes = size_t(c.nrows) * (c.kind == K_BOOL ? 1 : 8);
        const size_t bbytes = c.expect > 0 ? size_t(c.expect) : 0;
        c.vals.reset(new uint8_t[vbytes]);
        c.block.reset(new uint8_t[bbytes]);
        if (!read_exact(f, c.vals.get(), vbytes)) return 2;
        if (c.has_valid) {
            c.valid.reset(new uint8_t[c.nrows]);
            if (!read_exact(f, c.valid.get(), c.nrows)) return 2;
        }
        if (!read_exact(f, c.block.get(), bbytes)) return 2;
        bad += check(c, int(ci), false);
        nenc++;
        if (c.kind == K_TS || c.kind == K_I64) {
            bad += check(c, int(ci), true);
            nenc++;
        }
    }
    fclose(f);
    printf("%u cases, %d encodes, %d failures\n", ncases, nenc, bad);
    return bad ? 1 : 0;
}
