/* Host check of the string page decoder (cnosdb_amd/csrc/gs_str_dec.h),
 * built with AddressSanitizer and UBSan by tests/test_str_decode_cpu.py.
 *
 * Input file (little-endian), written by tests/str_corpus.py:
 *   u32 ncases
 *   per case: u32 name_len, name; u32 data_len, data; u32 nrows;
 *             u32 all_valid; (nrows+7)/8 validity bytes; u32 reject;
 *             u64 payload_len; unless reject: nrows i64 lengths (-1 = null),
 *             then the bytes of all rows back to back
 *
 * Every page's data sits in a heap block of exactly data_len bytes and is
 * decoded into a heap slab of exactly str_slab_size bytes, as the engine
 * lays it out, so any access outside either is an ASan error.  Checked per
 * case: the slab size lies in [payload_len, what the stream can produce];
 * the rows are byte-equal to the expectation, or the page is rejected; and
 * a page whose preamble exceeds its slab leaves every slab byte untouched. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gs_str_dec.h"

static bool read_exact(FILE *f, void *dst, size_t n) {
    return n == 0 || fread(dst, 1, n, f) == n;
}

struct Case {
    std::string name;
    uint32_t data_len = 0, nrows = 0, all_valid = 0, reject = 0;
    uint64_t payload_len = 0;
    std::unique_ptr<uint8_t[]> data, bits;
    std::vector<int64_t> lens;
    std::vector<uint8_t> bytes;
};

static bool read_case(FILE *f, Case &c) {
    uint32_t nl = 0;
    if (!read_exact(f, &nl, 4)) return false;
    c.name.resize(nl);
    if (!read_exact(f, &c.name[0], nl)) return false;
    if (!read_exact(f, &c.data_len, 4)) return false;
    c.data.reset(new uint8_t[c.data_len]);
    if (!read_exact(f, c.data.get(), c.data_len)) return false;
    if (!read_exact(f, &c.nrows, 4) || !read_exact(f, &c.all_valid, 4))
        return false;
    const size_t nb = (size_t(c.nrows) + 7) / 8;
    c.bits.reset(new uint8_t[nb]);
    if (!read_exact(f, c.bits.get(), nb)) return false;
    if (!read_exact(f, &c.reject, 4) || !read_exact(f, &c.payload_len, 8))
        return false;
    if (c.reject) return true;
    c.lens.resize(c.nrows);
    if (!read_exact(f, c.lens.data(), size_t(c.nrows) * 8)) return false;
    size_t total = 0;
    for (int64_t l : c.lens) total += l > 0 ? size_t(l) : 0;
    c.bytes.resize(total);
    return read_exact(f, c.bytes.data(), total);
}

#define FILL 0xA5

static int check_case(const Case &c) {
    const uint8_t *data = c.data.get();
    const uint8_t enc = c.data_len ? data[0] : 0;
    const uint64_t slab = str_slab_size(data, c.data_len, enc);
    /* less than 22 bytes out per stream byte, see str_slab_bound */
    uint64_t bound = 0;
    if (enc == STR_ENC_SNAPPY && c.data_len > 2)
        bound = 22 * (uint64_t(c.data_len) - 2);
    else if (enc == STR_ENC_NULL)
        bound = c.data_len - 1;
    if (slab > bound || (!c.reject && slab < c.payload_len)) {
        printf("%s: slab %llu outside [%llu, %llu]\n", c.name.c_str(),
               (unsigned long long)slab, (unsigned long long)c.payload_len,
               (unsigned long long)bound);
        return 1;
    }
    std::unique_ptr<uint8_t[]> buf(new uint8_t[slab]);
    memset(buf.get(), FILL, slab);
    std::unique_ptr<int64_t[]> sz(new int64_t[c.nrows]);
    std::unique_ptr<int64_t[]> pos(new int64_t[c.nrows]);
    std::unique_ptr<uint8_t[]> valid(new uint8_t[c.nrows]);
    const unsigned e = str_page_decode(
        data, c.data_len, enc, c.bits.get(), int(c.all_valid), c.nrows,
        buf.get(), 0, sz.get(), pos.get(), valid.get());
    uint64_t pre = 0;
    if (enc == STR_ENC_SNAPPY && c.data_len > 2 &&
        str_varint(data + 2, uint64_t(c.data_len) - 2, &pre) && pre > slab) {
        for (uint64_t k = 0; k < slab; k++)
            if (buf[k] != FILL) {
                printf("%s: slab byte %llu written though the preamble "
                       "exceeds the slab\n", c.name.c_str(),
                       (unsigned long long)k);
                return 1;
            }
    }
    if (c.reject) {
        if (e == STR_OK) {
            printf("%s: accepted, must be rejected\n", c.name.c_str());
            return 1;
        }
        return 0;
    }
    if (e != STR_OK) {
        printf("%s: rejected (%u), must decode\n", c.name.c_str(), e);
        return 1;
    }
    size_t at = 0;
    for (uint32_t r = 0; r < c.nrows; r++) {
        const int64_t want = c.lens[r];
        if (want < 0) {
            if (valid[r] || sz[r] != 0) {
                printf("%s: row %u not null\n", c.name.c_str(), r);
                return 1;
            }
            continue;
        }
        if (!valid[r] || sz[r] != want || pos[r] < 0 ||
            uint64_t(pos[r]) + uint64_t(want) > slab ||
            (want > 0 && memcmp(buf.get() + pos[r], c.bytes.data() + at,
                                size_t(want)))) {
            printf("%s: row %u differs\n", c.name.c_str(), r);
            return 1;
        }
        at += size_t(want);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2 && argc != 3) {
        fprintf(stderr, "usage: %s <cases file> [-v]\n", argv[0]);
        return 2;
    }
    const bool verbose = argc == 3; /* name each case before it runs, so a
                                       sanitizer abort can be placed */
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4)) return 2;
    int bad = 0, nwell = 0, nmal = 0;
    for (uint32_t i = 0; i < ncases; i++) {
        Case c;
        if (!read_case(f, c)) {
            fprintf(stderr, "case %u: short file\n", i);
            return 2;
        }
        if (verbose) {
            printf("case %s\n", c.name.c_str());
            fflush(stdout);
        }
        bad += check_case(c);
        if (c.reject) nmal++; else nwell++;
    }
    fclose(f);
    printf("%d well-formed pages, %d malformed pages, %d failures\n", nwell,
           nmal, bad);
    return bad ? 1 : 0;
}
