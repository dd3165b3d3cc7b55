/* The cell rules of gs_agg_group: the bucket index of a row, the partial
 * record of one (cell, column) and the two ways it grows: by one row
 * (agg_add_row) and by another partial (agg_combine).  The aggregate kernels
 * of gs_engine.cpp and the entry point go through it; the header also
 * compiles as host C++ (tests/cpu/agg_check.cpp), where the same code runs
 * under AddressSanitizer and UBSan.
 *
 * A partial carries, next to the six aggregates, the ROW INDEX that holds
 * each order-dependent one (min, max, first, last).  With them every rule of
 * the contract is a lexicographic extremum:
 *   min    smallest value by the strict compare of the column's type, among
 *          equal values (+0.0 == -0.0) the lowest row
 *   max    likewise with the largest value
 *   first  smallest (timestamp, row)
 *   last   largest (timestamp, row)
 * so agg_combine is associative AND commutative in every field but the f64
 * sum, and a fold of the rows one by one in row order gives exactly the
 * sequential strict-compare loop the contract describes (a later row never
 * displaces an equal earlier one; NaN compares false both ways and never
 * enters a bound).  The f64 sum is IEEE addition, commutative but not
 * associative: its bits depend on the shape of the fold, nothing else does.
 *
 * Plain integer/float code, no atomics, LDS or lane intrinsics. */
#ifndef GS_AGG_H
#define GS_AGG_H

#include <cstdint>
#include "gs_filter.h" /* FLT_FN, flt_f64, GS_CT_* */

/* ------------------------------------------------------------ the buckets */

/* Where a row stands on the bucket axis of its series.  Returns whether the
 * row is in a bucket; *slot is that bucket, or for a row in none the bucket
 * it sorts next to (0 before t0, n_buckets - 1 behind the last), so that
 * (series, slot) never decreases along a sorted series.  bucket_ns == 0 is
 * one bucket that holds every row, whatever t0.  ts - t0 is formed in
 * uint64, where it cannot overflow: for ts >= t0 the true difference lies in
 * [0, 2^64). */
FLT_FN bool agg_slot(uint64_t b, int32_t n_buckets, int32_t *slot) {
    if (b >= uint64_t(n_buckets)) { *slot = n_buckets - 1; return false; }
    *slot = int32_t(b);
    return true;
}

/* The unbounded bucket index b = uint64(ts - t0) / bucket_ns; false for a
 * row in front of t0.  The one place that divides. */
FLT_FN bool agg_bucket_raw(int64_t ts, int64_t t0, int64_t bucket_ns,
                           uint64_t *b) {
    *b = 0;
    if (bucket_ns == 0) return true;
    if (ts < t0) return false;
    *b = (uint64_t(ts) - uint64_t(t0)) / uint64_t(bucket_ns);
    return true;
}

FLT_FN bool agg_bucket(int64_t ts, int64_t t0, int64_t bucket_ns,
                       int32_t n_buckets, int32_t *slot) {
    uint64_t b;
    if (!agg_bucket_raw(ts, t0, bucket_ns, &b)) { *slot = 0; return false; }
    return agg_slot(b, n_buckets, slot);
}

/* The same index without a division, from a bucket already known: d is
 * uint64(ts - t0) of a row with ts >= t0, [wlo, wlo + bucket_ns) the window
 * of bucket wb.  Answers when d lies in that window or the next one;
 * otherwise (a jump of more than one bucket, or d in front of the window)
 * returns false and the caller divides. */
FLT_FN bool agg_bucket_near(uint64_t d, uint64_t wlo, uint64_t wb,
                            uint64_t bucket_ns, uint64_t *b) {
    if (d < wlo) return false;
    const uint64_t delta = d - wlo;
    if (delta < bucket_ns) { *b = wb; return true; }
    if (delta - bucket_ns < bucket_ns) { *b = wb + 1; return true; }
    return false;
}

/* ------------------------------------------------------------ the partial */

#define AGG_NFIELD 12 /* 8-byte words of an AggPart, in declaration order */

struct AggPart {
    int64_t count;      /* valid cells folded in */
    uint64_t sum;       /* raw bits in the column's sum type */
    uint64_t mn, mx;    /* raw bits in the column's type */
    int64_t mn_row, mx_row;
    uint64_t first, last;
    int64_t first_ts, last_ts;
    int64_t first_row, last_row;
};

FLT_FN uint64_t agg_f64_bits(double d) {
    uint64_t b;
    __builtin_memcpy(&b, &d, 8);
    return b;
}

/* The partial of no cell at all: what an empty output cell holds. */
FLT_FN AggPart agg_empty(int ctype) {
    AggPart p;
    p.count = 0;
    p.sum = 0;
    if (ctype == GS_CT_F64) {
        p.mn = 0x7ff0000000000000ULL; /* +inf */
        p.mx = 0xfff0000000000000ULL; /* -inf */
    } else if (ctype == GS_CT_I64) {
        p.mn = uint64_t(INT64_MAX);
        p.mx = uint64_t(INT64_MIN);
    } else if (ctype == GS_CT_BOOL) {
        p.mn = 1;
        p.mx = 0;
    } else {
        p.mn = UINT64_MAX;
        p.mx = 0;
    }
    p.mn_row = INT64_MAX;
    p.mx_row = INT64_MAX;
    p.first = p.last = 0;
    p.first_ts = INT64_MAX;
    p.last_ts = INT64_MIN;
    p.first_row = INT64_MAX;
    p.last_row = -1;
    return p;
}

/* a < b by the strict compare of the column's type */
FLT_FN bool agg_lt(int ctype, uint64_t a, uint64_t b) {
    if (ctype == GS_CT_F64) return flt_f64(a) < flt_f64(b);
    if (ctype == GS_CT_I64) return int64_t(a) < int64_t(b);
    return a < b;
}
FLT_FN bool agg_eq(int ctype, uint64_t a, uint64_t b) {
    if (ctype == GS_CT_F64) return flt_f64(a) == flt_f64(b);
    return a == b;
}

/* Fold `r` into `l`.  The contract's wording has l precede r in row order;
 * by the row indices the result does not depend on which side is which,
 * except for the rounding of an f64 sum of three or more pieces. */
FLT_FN AggPart agg_combine(int ctype, const AggPart &l, const AggPart &r) {
    AggPart o = l;
    o.count = int64_t(uint64_t(l.count) + uint64_t(r.count));
    if (ctype == GS_CT_F64)
        o.sum = agg_f64_bits(flt_f64(l.sum) + flt_f64(r.sum));
    else
        o.sum = l.sum + r.sum; /* exact modulo 2^64 */
    if (agg_lt(ctype, r.mn, l.mn) ||
        (agg_eq(ctype, r.mn, l.mn) && r.mn_row < l.mn_row)) {
        o.mn = r.mn;
        o.mn_row = r.mn_row;
    }
    if (agg_lt(ctype, l.mx, r.mx) ||
        (agg_eq(ctype, r.mx, l.mx) && r.mx_row < l.mx_row)) {
        o.mx = r.mx;
        o.mx_row = r.mx_row;
    }
    if (r.first_ts < l.first_ts ||
        (r.first_ts == l.first_ts && r.first_row < l.first_row)) {
        o.first = r.first;
        o.first_ts = r.first_ts;
        o.first_row = r.first_row;
    }
    if (r.last_ts > l.last_ts ||
        (r.last_ts == l.last_ts && r.last_row > l.last_row)) {
        o.last = r.last;
        o.last_ts = r.last_ts;
        o.last_row = r.last_row;
    }
    return o;
}

/* The partial of one valid cell: value bits in the column's type (a bool's
 * byte zero-extended), its timestamp and its row in the set. */
FLT_FN AggPart agg_single(int ctype, uint64_t bits, int64_t ts, int64_t row) {
    AggPart p = agg_empty(ctype);
    p.count = 1;
    p.sum = bits; /* bool: 0/1, so the sum counts the true cells */
    /* a NaN enters neither bound: the bound keeps its start value and the
       row of no cell */
    if (ctype != GS_CT_F64 || flt_f64(bits) == flt_f64(bits)) {
        p.mn = p.mx = bits;
        p.mn_row = p.mx_row = row;
    }
    p.first = p.last = bits;
    p.first_ts = p.last_ts = ts;
    p.first_row = p.last_row = row;
    return p;
}

FLT_FN void agg_add_row(AggPart &p, int ctype, uint64_t bits, int64_t ts,
                        int64_t row) {
    p = agg_combine(ctype, p, agg_single(ctype, bits, ts, row));
}

#endif /* GS_AGG_H */
