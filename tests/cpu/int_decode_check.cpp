/* Host check of the integer and bool page decoders
 * (cnosdb_amd/csrc/gs_int_dec.h), built with AddressSanitizer and UBSan by
 * tests/test_int_decode_cpu.py.
 *
 * Input file (little-endian), written by tests/int_corpus.py:
 *   u32 ncases
 *   per case: u32 name_len, name; u32 kind (0 ts, 1 i64, 2 bool);
 *             u32 data_len, data; u32 nrows; u32 all_valid;
 *             (nrows+7)/8 validity bytes; u32 flags (1 reject, 2 nonmono,
 *             4 print the header); unless reject: nrows i64 values, then
 *             nrows validity bytes
 *
 * Every page's data and bitset sit in heap blocks of exactly their lengths
 * and the outputs in blocks of exactly nrows, so any access outside them is
 * an ASan error.  Checked per case: the page is rejected (FORMAT or SHORT)
 * exactly when the file says so; a decoded page equals the expectation in
 * values and validity, and raises NONMONO exactly when declared.  A case
 * flagged 4 prints "hdr <name> <first> <rle_delta>" from int_page_header. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "gs_int_dec.h"

enum { F_REJECT = 1, F_NONMONO = 2, F_HEADER = 4 };
enum { K_TS = 0, K_I64 = 1, K_BOOL = 2 };

static bool read_exact(FILE *f, void *dst, size_t n) {
    return n == 0 || fread(dst, 1, n, f) == n;
}

struct Case {
    std::string name;
    uint32_t kind = 0, data_len = 0, nrows = 0, all_valid = 0, flags = 0;
    std::unique_ptr<uint8_t[]> data, bits;
    std::vector<int64_t> values;
    std::vector<uint8_t> valid;
};

static bool read_case(FILE *f, Case &c) {
    uint32_t nl = 0;
    if (!read_exact(f, &nl, 4)) return false;
    c.name.resize(nl);
    if (!read_exact(f, &c.name[0], nl)) return false;
    if (!read_exact(f, &c.kind, 4) || !read_exact(f, &c.data_len, 4))
        return false;
    c.data.reset(new uint8_t[c.data_len]);
    if (!read_exact(f, c.data.get(), c.data_len)) return false;
    if (!read_exact(f, &c.nrows, 4) || !read_exact(f, &c.all_valid, 4))
        return false;
    const size_t nb = (size_t(c.nrows) + 7) / 8;
    c.bits.reset(new uint8_t[nb]);
    if (!read_exact(f, c.bits.get(), nb)) return false;
    if (!read_exact(f, &c.flags, 4)) return false;
    if (c.flags & F_REJECT) return true;
    c.values.resize(c.nrows);
    c.valid.resize(c.nrows);
    return read_exact(f, c.values.data(), size_t(c.nrows) * 8) &&
           read_exact(f, c.valid.data(), c.nrows);
}

static int check_case(const Case &c) {
    const uint8_t *data = c.data.get();
    const uint8_t enc = c.data_len ? data[0] : 0;
    std::unique_ptr<int64_t[]> out(new int64_t[c.nrows]);
    std::unique_ptr<uint8_t[]> bout(new uint8_t[c.nrows]);
    std::unique_ptr<uint8_t[]> valid(new uint8_t[c.nrows]);
    unsigned e;
    if (c.kind == K_BOOL) {
        e = bool_page_decode(data, c.data_len, enc, c.bits.get(),
                             int(c.all_valid), c.nrows, bout.get(),
                             valid.get());
        for (uint32_t r = 0; r < c.nrows; r++) out[r] = bout[r];
    } else {
        e = int_page_decode(data, c.data_len, enc, c.kind == K_TS,
                            c.bits.get(), int(c.all_valid), c.nrows,
                            out.get(), valid.get());
    }
    if (c.flags & F_HEADER) {
        const IntHeader h = int_page_header(data, c.data_len, enc);
        printf("hdr %s %lld %lld\n", c.name.c_str(), (long long)h.first,
               (long long)h.rle_delta);
    }
    const bool rejected = e & (INT_ERR_FORMAT | INT_ERR_SHORT);
    if (c.flags & F_REJECT) {
        if (!rejected) {
            printf("%s: accepted, must be rejected\n", c.name.c_str());
            return 1;
        }
        return 0;
    }
    if (rejected) {
        printf("%s: rejected (%u), must decode\n", c.name.c_str(), e);
        return 1;
    }
    if (bool(e & INT_ERR_NONMONO) != bool(c.flags & F_NONMONO)) {
        printf("%s: non-monotonic verdict %u, declared %u\n", c.name.c_str(),
               e & INT_ERR_NONMONO, c.flags & F_NONMONO);
        return 1;
    }
    for (uint32_t r = 0; r < c.nrows; r++)
        if (out[r] != c.values[r] || valid[r] != c.valid[r]) {
            printf("%s: row %u is %lld/%u, expected %lld/%u\n",
                   c.name.c_str(), r, (long long)out[r], valid[r],
                   (long long)c.values[r], c.valid[r]);
            return 1;
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
    int bad = 0, ndec = 0, nrej = 0;
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
        if (c.flags & F_REJECT) nrej++; else ndec++;
    }
    fclose(f);
    printf("%d decoded pages, %d rejected pages, %d failures\n", ndec, nrej,
           bad);
    return bad ? 1 : 0;
}
