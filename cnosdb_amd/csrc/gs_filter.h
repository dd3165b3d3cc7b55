/* The cell rules of gs_filter_group: the single home of the typed compare
 * of one cell against a predicate, of "a timestamp lies in a deleted range"
 * and of the normal form of a range list.  The filter kernels of
 * gs_engine.cpp and the entry point go through it; the header also compiles
 * as host C++ (tests/cpu/filter_check.cpp), where the same code runs under
 * AddressSanitizer and UBSan on exact-size buffers.
 *
 * Semantics mirror:
 *   tskv/src/reader/filter.rs:91-142   DataFilter: the pushed expression is
 *       evaluated over the batch in each column's own type, a comparison
 *       with a null cell is null, and filter_record_batch drops the rows
 *       whose mask is null or false
 *   tskv/src/tsm/reader.rs:634-656     update_nullbits_by_time_range: a
 *       deleted range is closed, min_ts <= ts <= max_ts
 *
 * Plain integer/float code, no atomics, LDS or lane intrinsics. */
#ifndef GS_FILTER_H
#define GS_FILTER_H

#include <cstdint>
#include "../../include/cnosdb_gs.h" /* GsTimeRange, GS_PRED_*, GS_CT_* */

#ifdef __HIPCC__
#define FLT_FN __host__ __device__ __forceinline__
#else
#define FLT_FN inline
#endif

/* ------------------------------------------------------------ the compare */

/* One comparison in type T.  For double these are the IEEE operators: NaN
 * fails everything but NE, and -0.0 == +0.0 (the rule of dev_pred_t<double>
 * in gs_scan's kernels, so both entries agree on every input). */
template <typename T>
FLT_FN bool flt_cmp(int op, T a, T b, T x) {
    switch (op) {
    case GS_PRED_GT: return x > a;
    case GS_PRED_GE: return x >= a;
    case GS_PRED_LT: return x < a;
    case GS_PRED_LE: return x <= a;
    case GS_PRED_EQ: return x == a;
    case GS_PRED_NE: return x != a;
    case GS_PRED_BETWEEN: return x >= a && x <= b;
    default: return false;
    }
}

FLT_FN double flt_f64(uint64_t bits) {
    double d;
    __builtin_memcpy(&d, &bits, 8);
    return d;
}

/* May this op stand in a GsColPred? */
FLT_FN bool flt_op_known(int op) {
    return op >= GS_PRED_GT && op <= GS_PRED_IS_NOT_NULL;
}
FLT_FN bool flt_op_is_null_test(int op) {
    return op == GS_PRED_IS_NULL || op == GS_PRED_IS_NOT_NULL;
}

/* Verdict of one cell.  x_bits: the cell's value as raw bits in the column's
 * type (a bool's byte zero-extended); valid: the cell's EFFECTIVE validity.
 * The two null tests never look at x_bits; a comparison on a null cell
 * fails.  i64 compares signed, u64 and bool unsigned, f64 by flt_cmp<double>;
 * the constants are raw bits in the same type, so nothing passes through a
 * double on the way. */
FLT_FN bool flt_cell(int op, int ctype, uint64_t a_bits, uint64_t b_bits,
                     uint64_t x_bits, bool valid) {
    if (op == GS_PRED_IS_NULL) return !valid;
    if (op == GS_PRED_IS_NOT_NULL) return valid;
    if (!valid) return false;
    if (ctype == GS_CT_F64)
        return flt_cmp<double>(op, flt_f64(a_bits), flt_f64(b_bits),
                               flt_f64(x_bits));
    if (ctype == GS_CT_I64)
        return flt_cmp<int64_t>(op, int64_t(a_bits), int64_t(b_bits),
                                int64_t(x_bits));
    return flt_cmp<uint64_t>(op, a_bits, b_bits, x_bits);
}

/* ------------------------------------------------------------ range lists */

/* Normal form of a list of closed ranges, in place: ranges with min > max
 * dropped, the rest sorted by min_ts, overlapping and touching ranges
 * ([1,5],[6,9] -> [1,9]) merged.  Returns the new count.  Afterwards the
 * ranges are disjoint, non-adjacent and increasing, which is what
 * flt_in_ranges searches. */
FLT_FN void flt_sift(GsTimeRange *r, int64_t root, int64_t n) {
    for (;;) {
        int64_t c = 2 * root + 1;
        if (c >= n) return;
        if (c + 1 < n && r[c].min_ts < r[c + 1].min_ts) c++;
        if (r[root].min_ts >= r[c].min_ts) return;
        const GsTimeRange t = r[root];
        r[root] = r[c];
        r[c] = t;
        root = c;
    }
}

FLT_FN int64_t flt_normalise(GsTimeRange *r, int64_t n) {
    int64_t m = 0;
    for (int64_t i = 0; i < n; i++)
        if (r[i].min_ts <= r[i].max_ts) r[m++] = r[i];
    /* heapsort by min_ts: in place, no recursion, O(m log m) */
    for (int64_t i = m / 2 - 1; i >= 0; i--) flt_sift(r, i, m);
    for (int64_t e = m - 1; e > 0; e--) {
        const GsTimeRange t = r[0];
        r[0] = r[e];
        r[e] = t;
        flt_sift(r, 0, e);
    }
    int64_t k = 0;
    for (int64_t i = 0; i < m; i++) {
        /* r[i].min_ts - 1 is only formed when min_ts > r[k-1].max_ts, so it
           cannot wrap below INT64_MIN; max_ts + 1 is never formed */
        if (k > 0 && (r[i].min_ts <= r[k - 1].max_ts ||
                      r[i].min_ts - 1 == r[k - 1].max_ts)) {
            if (r[i].max_ts > r[k - 1].max_ts) r[k - 1].max_ts = r[i].max_ts;
        } else {
            r[k++] = r[i];
        }
    }
    return k;
}

/* Does ts lie in one of the n ranges of a NORMALISED list?  Binary search
 * for the last range that starts at or before ts. */
FLT_FN bool flt_in_ranges(const GsTimeRange *r, int n, int64_t ts) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int m = (lo + hi) >> 1;
        if (r[m].min_ts <= ts) lo = m + 1; else hi = m;
    }
    return lo > 0 && ts <= r[lo - 1].max_ts;
}

#endif /* GS_FILTER_H */
