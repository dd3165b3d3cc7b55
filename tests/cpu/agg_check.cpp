/* Host check of the cell rules of gs_agg_group (cnosdb_amd/csrc/gs_agg.h),
 * built with AddressSanitizer and UBSan by tests/test_agg_cpu.py.
 *
 * Input file (little-endian), written by tests/agg_ref.py:
 *   u32 nruns
 *   per run: i32 ctype, u32 nrows,
 *            nrows x (i64 ts, u64 value bits, i64 row, u32 effective validity),
 *            the expected cell: i64 count, u64 sum, min, max, first, last,
 *            i64 first_ts, last_ts; f64 sum of |x| (the f64 sum's tolerance)
 *   u32 nprobes
 *   per probe: i64 ts, t0, bucket_ns; i32 n_buckets, in a bucket, bucket
 *
 * A run is the rows of one cell in row order, in a heap block of exactly
 * its size.  Checked per run:
 *   - the fold of the valid rows one by one (agg_add_row) equals the
 *     expected cell: every field bit for bit, an f64 sum within
 *     count * 2^-53 * sum|x| of the reference (NaN and infinities in kind)
 *   - every split into 2 and into 3 consecutive pieces, each folded row by
 *     row and joined with agg_combine (three pieces in both groupings, two
 *     also with the sides exchanged), and the splits into 2..5 pieces of
 *     rows that many apart (how lanes of a wave own rows), give the SAME
 *     BITS as the fold one by one in every field of the partial, the row
 *     indices included, except the f64 sum, which stays within the bound
 * Checked per probe: agg_bucket's verdict and slot; and, between any two
 * probes of one bucket layout, that agg_bucket_near either declines or
 * gives the index agg_bucket_raw divides out. */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gs_agg.h"

struct Row {
    int64_t ts;
    uint64_t bits;
    int64_t row;
    uint32_t valid;
};

static bool read_exact(FILE *f, void *dst, size_t n) {
    return n == 0 || fread(dst, 1, n, f) == n;
}

static AggPart fold(int ct, const Row *rows, size_t a, size_t b,
                    size_t step = 1) {
    AggPart p = agg_empty(ct);
    for (size_t i = a; i < b; i += step)
        if (rows[i].valid) agg_add_row(p, ct, rows[i].bits, rows[i].ts, rows[i].row);
    return p;
}

static bool sum_ok(int ct, uint64_t got, uint64_t ref, int64_t count,
                   double sum_abs) {
    if (ct != GS_CT_F64) return got == ref;
    const double g = flt_f64(got), r = flt_f64(ref);
    if (std::isnan(g) || std::isnan(r)) return std::isnan(g) && std::isnan(r);
    if (std::isinf(g) || std::isinf(r)) return g == r;
    return std::fabs(g - r) <= double(count) * 0x1p-53 * sum_abs;
}

/* every field but the sum, bit for bit */
static bool same_but_sum(const AggPart &a, const AggPart &b) {
    AggPart x = a, y = b;
    x.sum = y.sum = 0;
    return memcmp(&x, &y, sizeof(AggPart)) == 0;
}

struct Want {
    int64_t count;
    uint64_t sum, mn, mx, first, last;
    int64_t first_ts, last_ts;
    double sum_abs;
};

static int check_run(uint32_t idx, int ct, const Row *rows, size_t n,
                     const Want &w, long &splits) {
    int bad = 0;
    const AggPart f = fold(ct, rows, 0, n);
    if (f.count != w.count || f.mn != w.mn || f.mx != w.mx ||
        f.first != w.first || f.last != w.last || f.first_ts != w.first_ts ||
        f.last_ts != w.last_ts || !sum_ok(ct, f.sum, w.sum, w.count, w.sum_abs)) {
        printf("run %u (ctype %d, %zu rows): the fold differs from the "
               "reference: count %lld/%lld sum %llx/%llx min %llx/%llx max "
               "%llx/%llx first %llx/%llx last %llx/%llx first_ts %lld/%lld "
               "last_ts %lld/%lld\n", idx, ct, n, (long long)f.count,
               (long long)w.count, (unsigned long long)f.sum,
               (unsigned long long)w.sum, (unsigned long long)f.mn,
               (unsigned long long)w.mn, (unsigned long long)f.mx,
               (unsigned long long)w.mx, (unsigned long long)f.first,
               (unsigned long long)w.first, (unsigned long long)f.last,
               (unsigned long long)w.last, (long long)f.first_ts,
               (long long)w.first_ts, (long long)f.last_ts,
               (long long)w.last_ts);
        bad++;
    }
    auto hold = [&](const AggPart &p, const char *what, size_t i, size_t j) {
        splits++;
        if (same_but_sum(p, f) && sum_ok(ct, p.sum, w.sum, w.count, w.sum_abs) &&
            (ct == GS_CT_F64 || p.sum == f.sum))
            return;
        printf("run %u (ctype %d, %zu rows): %s at %zu, %zu differs from the "
               "fold row by row\n", idx, ct, n, what, i, j);
        bad++;
    };
    for (size_t i = 0; i <= n; i++) {
        const AggPart a = fold(ct, rows, 0, i), b = fold(ct, rows, i, n);
        hold(agg_combine(ct, a, b), "split in 2", i, n);
        hold(agg_combine(ct, b, a), "split in 2, sides exchanged", i, n);
        for (size_t j = i; j <= n; j++) {
            const AggPart m = fold(ct, rows, i, j), c = fold(ct, rows, j, n);
            hold(agg_combine(ct, agg_combine(ct, a, m), c),
                 "split in 3, (a b) c", i, j);
            hold(agg_combine(ct, a, agg_combine(ct, m, c)),
                 "split in 3, a (b c)", i, j);
        }
    }
    for (size_t k = 2; k <= 5; k++) {
        AggPart up = agg_empty(ct), down = agg_empty(ct);
        for (size_t p = 0; p < k; p++) {
            up = agg_combine(ct, up, fold(ct, rows, p, n, k));
            down = agg_combine(ct, fold(ct, rows, k - 1 - p, n, k), down);
        }
        hold(up, "rows k apart, pieces ascending", k, 0);
        hold(down, "rows k apart, pieces descending", k, 0);
    }
    return bad;
}

struct Probe {
    int64_t ts, t0, bn;
    int32_t nb, in, b;
};

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <cases file>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int bad = 0;
    long splits = 0;
    uint32_t nruns = 0, nprobes = 0;
    if (!read_exact(f, &nruns, 4)) return 2;
    for (uint32_t r = 0; r < nruns; r++) {
        int32_t ct;
        uint32_t n;
        if (!read_exact(f, &ct, 4) || !read_exact(f, &n, 4)) return 2;
        std::unique_ptr<Row[]> rows(new Row[n]);
        for (uint32_t i = 0; i < n; i++)
            if (!read_exact(f, &rows[i].ts, 8) || !read_exact(f, &rows[i].bits, 8) ||
                !read_exact(f, &rows[i].row, 8) || !read_exact(f, &rows[i].valid, 4))
                return 2;
        Want w;
        if (!read_exact(f, &w.count, 8) || !read_exact(f, &w.sum, 8) ||
            !read_exact(f, &w.mn, 8) || !read_exact(f, &w.mx, 8) ||
            !read_exact(f, &w.first, 8) || !read_exact(f, &w.last, 8) ||
            !read_exact(f, &w.first_ts, 8) || !read_exact(f, &w.last_ts, 8) ||
            !read_exact(f, &w.sum_abs, 8))
            return 2;
        bad += check_run(r, ct, rows.get(), n, w, splits);
    }
    if (!read_exact(f, &nprobes, 4)) return 2;
    std::vector<Probe> ps(nprobes);
    for (uint32_t i = 0; i < nprobes; i++)
        if (!read_exact(f, &ps[i].ts, 8) || !read_exact(f, &ps[i].t0, 8) ||
            !read_exact(f, &ps[i].bn, 8) || !read_exact(f, &ps[i].nb, 4) ||
            !read_exact(f, &ps[i].in, 4) || !read_exact(f, &ps[i].b, 4))
            return 2;
    fclose(f);
    long nears = 0;
    for (uint32_t i = 0; i < nprobes; i++) {
        const Probe &p = ps[i];
        int32_t slot = -7;
        const bool in = agg_bucket(p.ts, p.t0, p.bn, p.nb, &slot);
        const int32_t want_slot =
            p.in ? p.b : (p.bn != 0 && p.ts < p.t0 ? 0 : p.nb - 1);
        if (in != (p.in != 0) || slot != want_slot) {
            printf("probe %u: ts %lld t0 %lld bucket_ns %lld n %d: in %d slot "
                   "%d, expected in %d slot %d\n", i, (long long)p.ts,
                   (long long)p.t0, (long long)p.bn, p.nb, int(in), slot, p.in,
                   want_slot);
            bad++;
        }
        /* the window of every other probe of the same layout */
        uint64_t bi;
        if (p.bn == 0 || !agg_bucket_raw(p.ts, p.t0, p.bn, &bi)) continue;
        const uint64_t di = uint64_t(p.ts) - uint64_t(p.t0);
        for (uint32_t j = 0; j < nprobes; j++) {
            const Probe &q = ps[j];
            uint64_t bj, got;
            if (q.t0 != p.t0 || q.bn != p.bn || q.nb != p.nb ||
                !agg_bucket_raw(q.ts, q.t0, q.bn, &bj))
                continue;
            nears++;
            if (agg_bucket_near(di, bj * uint64_t(q.bn), bj, uint64_t(q.bn),
                                &got) && got != bi) {
                printf("probe %u from the window of probe %u: bucket %llu, "
                       "expected %llu\n", i, j, (unsigned long long)got,
                       (unsigned long long)bi);
                bad++;
            }
        }
    }
    printf("%u runs, %ld folds of pieces, %u probes, %ld window checks, "
           "%d failures\n", nruns, splits, nprobes, nears, bad);
    return bad ? 1 : 0;
}
