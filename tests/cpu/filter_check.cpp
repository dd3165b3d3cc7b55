/* Host check of the cell rules of gs_filter_group
 * (cnosdb_amd/csrc/gs_filter.h), built with AddressSanitizer and UBSan by
 * tests/test_filter_cpu.py.
 *
 * Input file (little-endian), written by tests/filter_ref.py:
 *   u32 ncells
 *   per cell: i32 op, i32 ctype, u64 a_bits, u64 b_bits, u64 x_bits,
 *             u32 effective validity, u32 expected verdict
 *   u32 nlists
 *   per list: u32 name_len, name; u32 n, n x (i64 min, i64 max) as given;
 *             u32 m, m x (i64 min, i64 max) the expected normal form;
 *             u32 nprobes, per probe: i64 ts, u32 expected membership
 *
 * Every list sits in a heap block of exactly its length, and the membership
 * search runs on a second block of exactly the normalised length, so any
 * access outside them is an ASan error.  Checked: flt_cell's verdict of
 * every cell; flt_normalise's count and ranges; flt_in_ranges of every
 * probe over the normalised list. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "gs_filter.h"

static bool read_exact(FILE *f, void *dst, size_t n) {
    return n == 0 || fread(dst, 1, n, f) == n;
}

static int check_cells(FILE *f, uint32_t n, int &bad) {
    for (uint32_t i = 0; i < n; i++) {
        int32_t op, ct;
        uint64_t a, b, x;
        uint32_t valid, expect;
        if (!read_exact(f, &op, 4) || !read_exact(f, &ct, 4) ||
            !read_exact(f, &a, 8) || !read_exact(f, &b, 8) ||
            !read_exact(f, &x, 8) || !read_exact(f, &valid, 4) ||
            !read_exact(f, &expect, 4))
            return 2;
        if (!flt_op_known(op)) {
            printf("cell %u: op %d is not known\n", i, op);
            bad++;
            continue;
        }
        const bool got = flt_cell(op, ct, a, b, x, valid != 0);
        if (got != (expect != 0)) {
            printf("cell %u: op %d ctype %d a %llx b %llx x %llx valid %u: "
                   "%d, expected %u\n", i, op, ct, (unsigned long long)a,
                   (unsigned long long)b, (unsigned long long)x, valid,
                   int(got), expect);
            bad++;
        }
    }
    return 0;
}

static int check_list(FILE *f, int &bad, uint32_t &nprobes) {
    uint32_t nl = 0, n = 0, m = 0, np = 0;
    if (!read_exact(f, &nl, 4)) return 2;
    std::string name(nl, '\0');
    if (!read_exact(f, &name[0], nl) || !read_exact(f, &n, 4)) return 2;
    std::unique_ptr<GsTimeRange[]> in(new GsTimeRange[n]);
    if (!read_exact(f, in.get(), size_t(n) * sizeof(GsTimeRange))) return 2;
    if (!read_exact(f, &m, 4)) return 2;
    std::unique_ptr<GsTimeRange[]> want(new GsTimeRange[m]);
    if (!read_exact(f, want.get(), size_t(m) * sizeof(GsTimeRange))) return 2;

    const int64_t k = flt_normalise(in.get(), n);
    bool same = k == int64_t(m);
    for (uint32_t i = 0; same && i < m; i++)
        same = in[i].min_ts == want[i].min_ts && in[i].max_ts == want[i].max_ts;
    if (!same) {
        printf("%s: normal form has %lld ranges, expected %u, or differs\n",
               name.c_str(), (long long)k, m);
        bad++;
    }
    /* the search sees a block of exactly the normalised size */
    const uint32_t kk = same ? m : 0;
    std::unique_ptr<GsTimeRange[]> norm(new GsTimeRange[kk]);
    if (kk) memcpy(norm.get(), in.get(), size_t(kk) * sizeof(GsTimeRange));
    if (!read_exact(f, &np, 4)) return 2;
    for (uint32_t i = 0; i < np; i++) {
        int64_t ts;
        uint32_t expect;
        if (!read_exact(f, &ts, 8) || !read_exact(f, &expect, 4)) return 2;
        if (!same) continue;
        const bool got = flt_in_ranges(norm.get(), int(kk), ts);
        if (got != (expect != 0)) {
            printf("%s: ts %lld membership %d, expected %u\n", name.c_str(),
                   (long long)ts, int(got), expect);
            bad++;
        }
    }
    nprobes += np;
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int bad = 0;
    uint32_t ncells = 0, nlists = 0, nprobes = 0;
    if (!read_exact(f, &ncells, 4) || check_cells(f, ncells, bad)) {
        fprintf(stderr, "short file (cells)\n");
        return 2;
    }
    if (!read_exact(f, &nlists, 4)) return 2;
    for (uint32_t i = 0; i < nlists; i++)
        if (check_list(f, bad, nprobes)) {
            fprintf(stderr, "short file (list %u)\n", i);
            return 2;
        }
    fclose(f);
    printf("%u cells, %u range lists, %u probes, %d failures\n", ncells,
           nlists, nprobes, bad);
    return bad ? 1 : 0;
}
