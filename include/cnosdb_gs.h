/* cnosdb_gs — C ABI of the MI355X-native TSM scan/decode engine.
 *
 * This is the drop-in seam described in SURVEY.md §8b: a thin host shim
 * standing where CnosDB's `ColumnGroupReader::read` + `decode_pages` stand
 * (tskv/src/reader/column_group/mod.rs:33-70,195-243 and
 * tskv/src/tsm/reader.rs:494-560) calls these entry points instead of the
 * Rust CPU codec path.  A Rust shim (cxx/bindgen) would reconstitute
 * RecordBatches zero-copy from the output buffers; INTEGRATION.md shows the
 * binding a cnosdb maintainer would add.
 *
 * Conventions:
 *  - all functions return 0 (GS_OK) on success or a negative GsStatus;
 *    gs_last_error() returns a thread-local message for the last failure.
 *  - device buffers are raw HIP device pointers owned by the caller
 *    (e.g. torch tensors); the library only allocates its internal page
 *    store and scratch.
 *  - one GsCtx per device; calls on a ctx are serialized on its HIP stream
 *    and synchronized before returning.
 */
#ifndef CNOSDB_GS_H
#define CNOSDB_GS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t GsStatus;
enum {
    GS_OK = 0,
    GS_ERR = -1,          /* generic; see gs_last_error() */
    GS_ERR_NO_GPU = -2,   /* HIP device unavailable — the product path never
                             falls back to CPU; callers must treat this as fatal */
    GS_ERR_FORMAT = -3,   /* malformed page / unknown encoding byte */
    GS_ERR_CRC = -4,      /* page crc32 mismatch (tsm/page.rs:58-76) */
    GS_ERR_CAP = -5,      /* output buffer too small */
    GS_ERR_SENTINEL = -6, /* Gorilla sentinel appeared as input (float.rs:58-60) */
};

/* Encoding byte, first byte of every encoded data buffer
 * (common/models/src/codec.rs:39-54) */
enum {
    GS_ENC_NULL = 1,
    GS_ENC_DELTA = 2,    /* i64: zigzag delta + simple8b/RLE  (codec/integer.rs) */
    GS_ENC_GORILLA = 6,  /* f64 XOR                           (codec/float.rs) */
    GS_ENC_SNAPPY = 7,   /* strings: snappy block             (codec/string.rs) */
    GS_ENC_BITPACK = 10, /* bool                              (codec/boolean.rs) */
    GS_ENC_DELTATS = 11, /* ts: delta + scaled simple8b/RLE   (codec/timestamp.rs) */
};

/* physical column type of a page (PhysicalCType, tsm/reader.rs:658-731) */
enum {
    GS_CT_TIME = 0, /* i64 timestamps */
    GS_CT_I64 = 1,
    GS_CT_F64 = 2,
    GS_CT_BOOL = 3,
    GS_CT_U64 = 4, /* bit-cast to i64, unsigned.rs:20-45 */
    GS_CT_STR = 5, /* snappy string blocks, codec/string.rs */
};

/* Closed time interval (common/models/src/predicate/domain.rs:36-44) */
typedef struct {
    int64_t min_ts;
    int64_t max_ts;
} GsTimeRange;

/* One on-disk page: bytes = [u32 BE bitset_len][u64 BE row_count]
 * [u32 BE crc32(data)][validity bitset, LSB-first][encoded data]
 * (tsm/page.rs:32-94); num_values mirrors PageMeta.num_values. */
typedef struct {
    const uint8_t *bytes;
    uint64_t len;
    uint32_t num_values;
    uint8_t ctype;    /* GS_CT_* */
    uint32_t column_id;
} GsPageSpec;

/* One column group = one series' time slab: a time page plus field pages,
 * all with the same row count (tsm/column_group.rs:10-17). */
typedef struct {
    const GsPageSpec *pages; /* pages[0] MUST be the time page */
    uint32_t npages;
    uint32_t series_id;
} GsColumnGroupDesc;

typedef struct GsCtx GsCtx;
typedef struct GsGroupSet GsGroupSet;

/* ---- context ---- */
GsCtx *gs_ctx_create(int device);
void gs_ctx_destroy(GsCtx *ctx);
const char *gs_last_error(void);
int gs_device_count(void);
const char *gs_version(void);

/* ---- write path (host): the re-encode side of the seam
 * (Page::arrow_array_to_page, tsm/page.rs:100-353 + codec encode fns).
 * Return encoded length, or a negative GsStatus. ---- */
int64_t gs_encode_ts(const int64_t *src, size_t n, uint8_t *dst, size_t cap);
int64_t gs_encode_i64(const int64_t *src, size_t n, uint8_t *dst, size_t cap);
int64_t gs_encode_f64(const double *src, size_t n, uint8_t *dst, size_t cap);
int64_t gs_encode_bool(const uint8_t *src, size_t n, uint8_t *dst, size_t cap);
/* string block: src = concatenated string bytes, lens[i] = byte length of
 * string i (non-null values only).  Produces [7][0x10][snappy raw] per
 * str_snappy_encode (codec/string.rs:32-88); empty input -> 0 bytes.
 * The snappy arithmetic restates the published algorithm of the
 * un-vendored `snap` crate v1.1.1, pinned by the reference's golden
 * vectors (string.rs:529-566). */
int64_t gs_encode_str(const uint8_t *src, const uint64_t *lens, int64_t nstr,
                      uint8_t *dst, size_t cap);
/* assemble a full page (header + crc + bitset + data), tsm/page.rs:488-497 */
int64_t gs_build_page(const uint8_t *bitset, int64_t nrows, const uint8_t *data,
                      size_t data_len, uint8_t *dst, size_t cap);
uint32_t gs_crc32(const uint8_t *data, size_t len); /* CRC-32/ISO-HDLC */

/* ---- device page store ----
 * Uploads raw page bytes of `ngroups` column groups to HBM and builds the
 * device-side page table.  validate_crc runs the crc32 check of
 * Page::crc_validation on upload (host-side).  Row layout: group g's rows
 * occupy [row_offset[g], row_offset[g] + num_values_g) in every output
 * column buffer; gs_set_rows returns the total. */
GsGroupSet *gs_groups_upload(GsCtx *ctx, const GsColumnGroupDesc *groups,
                             size_t ngroups, int validate_crc);
void gs_groups_free(GsGroupSet *set);
int64_t gs_set_rows(const GsGroupSet *set);
int64_t gs_set_groups(const GsGroupSet *set);
/* series-level group count (consecutive same-series groups merged) */
int64_t gs_set_series(const GsGroupSet *set);
/* pushed-down COUNT from page metadata (pushdown_agg_reader.rs:39-106) */
int64_t gs_count_pushdown(const GsGroupSet *set, uint32_t col);
/* copy the per-group row offsets (ngroups entries) into caller buffer */
GsStatus gs_set_row_offsets(const GsGroupSet *set, int64_t *out);

/* ---- decode (hot loop ①, tsm/reader.rs:494-560) ----
 * Decodes column slot `col` (index into each group's pages[]) of every
 * group into d_out (device, 8 B/row for i64/f64/u64, 1 B for bool) at the
 * group row offsets.  Null slots are written as 0 (arrow builder
 * append_null semantics).  d_valid (device, 1 B/row, may be NULL) receives
 * 1 for valid rows, 0 for null rows. */
GsStatus gs_decode(GsCtx *ctx, GsGroupSet *set, uint32_t col, void *d_out,
                   uint8_t *d_valid);

/* ---- memcache rows (MemCacheReader, tskv/src/reader/memcache_reader.rs;
 * rows from mem_cache/series_data.rs:15-27) ----
 * A raw row set gives the unflushed in-memory rows the same series
 * structure as a page set, with NO pages: counts[i] = rows of series i
 * (time-sorted, non-null — pre-filter nulls when building the arrays).
 * gs_scan over a raw set skips the decode phases and filters/aggregates
 * the caller's device-resident spec->d_ts / spec->d_val directly
 * (tombstones and value predicates apply as usual; the fused path never
 * runs).  Raw sets also feed gs_compact_merge, so hot (memcache) and
 * cold (TSM) streams dedup together — newest stream wins at equal ts. */
GsGroupSet *gs_raw_set(GsCtx *ctx, const int64_t *counts, int64_t nseries);

/* ---- string column decode (str_snappy_decode_to_array,
 * codec/string.rs:226-276 via data_buf_to_arrow_array,
 * tsm/reader.rs:658-731) ----
 * Decodes string column slot `col` of every group into Arrow
 * varbinary layout at the set's row offsets: d_offsets (device,
 * int64[rows+1], exclusive prefix of byte lengths; null rows
 * contribute 0) and d_bytes (device, capacity bytes_cap).  d_valid
 * (device, 1 B/row, may be NULL) gets the validity bytes.  On return
 * *total_bytes = d_offsets[rows].  A page whose payload ends while valid
 * rows remain fails the call (the reference's builder stops appending and
 * returns a shorter array; rows are never silently nulled), and so does
 * any malformed block.  Strings behind the last valid row are ignored.
 * Handles GS_ENC_SNAPPY and GS_ENC_NULL blocks; empty data region -> all
 * rows null.  Current limit: rows <= 134M per set for the device offset
 * scan. */
GsStatus gs_decode_str(GsCtx *ctx, GsGroupSet *set, uint32_t col,
                       int64_t *d_offsets, uint8_t *d_bytes,
                       int64_t bytes_cap, uint8_t *d_valid,
                       int64_t *total_bytes);

/* ---- tombstone masking (tsm/reader.rs:634-656) ----
 * Clears validity (in d_valid) for rows whose decoded timestamp (d_ts,
 * from gs_decode of the time page) falls in any deleted closed range.
 * Applied per group; `ranges` apply to every group in the set. */
GsStatus gs_apply_tombstone(GsCtx *ctx, GsGroupSet *set, const int64_t *d_ts,
                            uint8_t *d_valid, const GsTimeRange *ranges,
                            size_t nranges);

/* ---- fused time-range scan (hot loops ①+②+④) ----
 * For the TSBS-devops shape: schema = time page + one f64 field page per
 * group (col 1).  Pipeline per group, entirely on device:
 *   decode ts -> decode f64 -> closed-interval time filter
 *   -> EITHER compacted output (d_out_ts/d_out_val at gather offsets)
 *      OR per-bucket aggregates (max/sum/count, fused, no row output).
 * Mirrors TableScanStream semantics for a pure time-range predicate
 * (data_source/batch/tskv.rs:351-371 pushes exactly these) with the
 * downsampling aggregate that stock DataFusion would run above
 * (SURVEY.md §8a row "downsampling agg").
 */
/* Value predicate on the scanned f64 field, evaluated like DataFilter's
 * pushed PhysicalExpr (reader/filter.rs:91-142): rows kept iff the time
 * range AND the predicate hold; a null field value fails the predicate
 * (arrow comparison-with-null semantics), unlike the time-only filter
 * where null field rows survive. */
enum {
    GS_PRED_NONE = 0,
    GS_PRED_GT = 1,
    GS_PRED_GE = 2,
    GS_PRED_LT = 3,
    GS_PRED_LE = 4,
    GS_PRED_EQ = 5,
    GS_PRED_NE = 6,
    GS_PRED_BETWEEN = 7, /* closed [a, b] */
};

typedef struct {
    int32_t op; /* GS_PRED_* */
    double a;
    double b;   /* BETWEEN upper bound */
} GsValuePred;

typedef struct {
    GsTimeRange range;     /* closed; use INT64_MIN/MAX for no filter */
    /* column slot of the f64 field to scan (0 = the first field page,
       i.e. pages[1]).  A multi-metric query (TSBS cpu-max-all-8) scans
       the same set once per field, reusing the uploaded pages; spans are
       recomputed per call (cheap, time-only). */
    int32_t field_col;
    /* deleted time ranges (tombstones) applied to the field column's
       validity before filter/agg (tsm/reader.rs:529-544) */
    const GsTimeRange *tombstones;
    size_t n_tombstones;
    /* aggregate spec; n_buckets == 0 disables aggregation */
    int64_t bucket_ns;     /* e.g. 300_000_000_000 for 5-min buckets */
    int64_t t0;            /* bucket origin: bucket = (ts - t0) / bucket_ns */
    int32_t n_buckets;
    /* device outputs for aggregation (caller-allocated, e.g. torch):
       d_max must be pre-filled with -inf, d_sum/d_count with 0 */
    double *d_agg_max;
    double *d_agg_sum;
    long long *d_agg_count;
    /* device outputs for compaction; NULL to skip row materialization.
       capacity must be >= gs_set_rows(set) rows. */
    int64_t *d_out_ts;
    double *d_out_val;
    /* scratch/outputs the caller provides (device):
       d_ts: decoded time column (gs_set_rows rows)
       d_val: decoded f64 column (gs_set_rows rows) */
    int64_t *d_ts;
    double *d_val;
    /* optional value predicate (general path; disables the fused path) */
    GsValuePred value_pred;
} GsScanSpec;

typedef struct {
    int64_t out_rows;      /* rows selected by the time filter */
    int64_t decoded_rows;  /* total rows decoded (= gs_set_rows) */
    /* per-phase kernel times, ms, measured with HIP events on the engine
       stream (for roofline accounting) */
    double ms_decode_ts;
    double ms_decode_val;
    double ms_filter;
    double ms_compact;
    double ms_agg;
} GsScanResult;

GsStatus gs_scan(GsCtx *ctx, GsGroupSet *set, const GsScanSpec *spec,
                 GsScanResult *result);

/* Async variant of the fused scan: gs_scan_async enqueues the whole
 * fused pipeline (requires the fused-capable shape: RLE ts pages,
 * all-valid Gorilla field pages, no tombstones, compacted outputs — the
 * TSBS shape; `d_ts`/`d_val` scratch is not used) and returns without
 * synchronizing; gs_scan_wait synchronizes the ctx stream and fills the
 * result.  Lets a caller overlap sub-batches on two ctx streams (the
 * Gorilla decode is ALU-bound, the aggregate HBM-bound). */
/* GROUP BY tag over a completed aggregate scan: keys the
 * per-series bucket partials by the decoded varbinary tag column (tags
 * are SeriesKey members, constant within a series —
 * tskv/src/reader/series.rs:23-100; the group-by above TskvExec is stock
 * DataFusion hash-agg in the reference).  Outputs per-(tag, bucket)
 * max/sum/count in deterministic first-occurrence tag order;
 * tag_rep_row[gid] = a row index whose string value IS the tag.
 * Precondition: gs_scan with the same n_buckets, and gs_decode_str of
 * the tag column, both on this set. */
GsStatus gs_groupby_tag(GsCtx *ctx, GsGroupSet *set, int tag_col,
                        int n_buckets, double *d_out_max, double *d_out_sum,
                        long long *d_out_count, int64_t *tag_rep_row,
                        int cap_gids, int *out_ngids);

/* Fused scan of nf field columns over ONE span/ts pass (TSBS
 * cpu-max-all-8, BASELINE config #3; the reference decodes every
 * projected field column of the column group in one decode_pages pass,
 * tsm/reader.rs:494-560).  Fused-capable shapes only.  Output strides:
 * d_out_val + f*total_rows per field; d_agg_* + f*n_buckets per field. */
GsStatus gs_scan_fields(GsCtx *ctx, GsGroupSet *set, const GsScanSpec *spec,
                        const int32_t *field_cols, int nf,
                        GsScanResult *result);
/* async variant: pair with gs_scan_wait */
GsStatus gs_scan_fields_async(GsCtx *ctx, GsGroupSet *set,
                              const GsScanSpec *spec,
                              const int32_t *field_cols, int nf);

GsStatus gs_scan_async(GsCtx *ctx, GsGroupSet *set, const GsScanSpec *spec);
GsStatus gs_scan_wait(GsCtx *ctx, GsGroupSet *set, GsScanResult *result);

/* ---- GPU page re-encode (the write side of compaction/flush:
 * Page::arrow_array_to_page, tsm/page.rs:100-353 + tsm/writer.rs:249-314).
 * kind: 0 = ts (DeltaTs), 1 = i64 (Delta), 2 = f64 (Gorilla).  d_vals is a
 * device column; pages are [h_row_off[p], +h_rows[p]) slices.  Each full
 * page (header+crc+bitset+data; the data block comes from the functions
 * gs_encode_* run on the host, csrc/gs_tsm_enc.h, so it is theirs byte for
 * byte) is written at d_out + p*cap_per_page; h_lens receives encoded
 * lengths.
 * This is the one-column case of gs_encode_group_pages_dev (below): the
 * same kernels with kind 0/1/2 as GS_CT_TIME/I64/F64, the page statistics
 * dropped.  One thing is this entry's own: kind 0 and kind 1 both require
 * all-valid slices (the time column is never null, and an i64 page with a
 * null row is refused here, where the group entry encodes its non-null
 * values).  Null-carrying i64, u64 and bool columns, and the statistics,
 * are the group entry's.  A call that passes d_valid holds a dense scratch
 * column of 8 B per row (up to the last page's end) for its duration.
 *
 * Errors: GS_ERR (before any device work) for a NULL required pointer, a
 * kind outside 0..2, npages <= 0 or a negative h_rows / h_row_off entry;
 * GS_ERR_CAP (before any device work) when cap_per_page is below
 * the worst case for the longest page; GS_ERR_SENTINEL when an f64 page
 * holds the Gorilla sentinel as a non-first value, as gs_encode_f64
 * reports it; GS_ERR_FORMAT for a null row in a ts/i64 page.  On the last
 * two h_lens is still filled: the pages that failed have a negative
 * entry, every other page of the launch is complete and valid. */
GsStatus gs_encode_pages_dev(GsCtx *ctx, int32_t kind, const void *d_vals,
                             const uint8_t *d_valid, const int64_t *h_row_off,
                             const int32_t *h_rows, int32_t npages,
                             uint8_t *d_out, int64_t cap_per_page,
                             int64_t *h_lens);

/* ---- GPU re-encode of a whole column group (the write side that follows
 * gs_compact_merge_fields) ----
 * Takes the merged columns as that call leaves them — the time column plus
 * up to GS_MAX_MERGE_COLS i64/u64/f64/bool field columns, validity bytes
 * and all — and writes every page of every column, each the page of the
 * host path (gs_encode_* over the non-null values + gs_build_page), whose
 * encoders, CRC and page header are the same functions (csrc/gs_tsm_enc.h).
 * The page split h_row_off/h_rows is shared by all columns.  u64 is the
 * i64 codec over the same bits (codec/unsigned.rs:15-18); an all-null or
 * zero-row page has an empty data region.  Value slots of null rows are
 * never read: they may hold anything, the Gorilla sentinel included.
 *
 * h_info[c*npages + p] also receives the page's PageStatistics as
 * Page::arrow_array_to_page computes them (tsm/page.rs:137-290): a
 * sequential loop over the non-null values with strict compares, starting
 * from INT64_MAX/INT64_MIN (time, i64), UINT64_MAX/0 (u64) or
 * DBL_MAX/-DBL_MAX (f64).  So a NaN changes neither bound, of +0.0 and
 * -0.0 the extremum keeps the sign of the first in row order, and a page
 * without a non-null value reports the starting values.  bool has no
 * min/max (0).  The bits do not depend on the launch geometry.
 *
 * GS_ERR (with a message, before any device work) for ncols outside
 * 1..GS_MAX_ENCODE_COLS, a ctype other than the five above (strings stay
 * with gs_encode_str), npages <= 0 or a NULL required pointer;
 * GS_ERR_CAP when a cap_per_page[c] is below that column's worst case for
 * the longest page (ints and f64 as in gs_encode_pages_dev, bool
 * 16 + ceil(n/8) + 2 + 10 + ceil(n/8)).  After the launch:
 * GS_ERR_SENTINEL for a non-first non-null f64 equal to the Gorilla
 * sentinel, GS_ERR_FORMAT for a null row in a GS_CT_TIME column, ranked
 * as in gs_encode_pages_dev.  h_info is then still filled: exactly the
 * failed (column, page) cells have len < 0, every other cell is complete
 * and valid. */
#define GS_MAX_ENCODE_COLS 33 /* time + GS_MAX_MERGE_COLS fields */

typedef struct {
    int64_t len;        /* full page length; negative = this page failed */
    int64_t null_count; /* rows - non-null rows */
    uint64_t min_bits;  /* raw bits in the column's type; 0 for bool */
    uint64_t max_bits;
} GsPageInfo;

GsStatus gs_encode_group_pages_dev(
    GsCtx *ctx, int32_t ncols,
    const uint8_t *ctype,          /* [ncols] GS_CT_TIME/I64/F64/BOOL/U64 */
    const void *const *d_vals,     /* [ncols] 8 B/row; bool 1 B/row (gs_decode widths) */
    const uint8_t *const *d_valid, /* [ncols] 1 B/row; entry or array NULL = all valid */
    const int64_t *h_row_off, const int32_t *h_rows, int32_t npages,
    uint8_t *const *d_out,         /* [ncols]; page p of column c at
                                      d_out[c] + p*cap_per_page[c] */
    const int64_t *cap_per_page,   /* [ncols] */
    GsPageInfo *h_info);           /* [ncols*npages], index c*npages + p */

/* ---- GPU re-encode of a string column's pages ----
 * The DataType::Utf8 arm of Page::arrow_array_to_page (tsm/page.rs:299-325)
 * on the device: the column in Arrow varbinary layout, as gs_decode_str
 * leaves it (d_offsets int64[rows + 1], d_bytes, d_valid 1 B/row), cut into
 * the pages h_row_off/h_rows.  Page p at d_out + p*cap_per_page is the page
 * of the host path byte for byte: gs_encode_str over the non-null strings
 * (codec/string.rs:32-88; the same source, csrc/gs_str_enc.h) under
 * gs_build_page, with the LSB-first validity bitset.  A zero-row or
 * all-null page has an empty data region.  Bytes of null rows are never
 * read, whatever length the offsets give them.
 *
 * h_info[p].len and null_count are as in gs_encode_group_pages_dev.  The
 * reference keeps a string page's min and max as byte strings
 * (PageStatistics::Bytes, page.rs:313-324), which do not fit 64 bits, so
 * min_bits / max_bits hold the ABSOLUTE ROW INDEX in the column of a row
 * whose value is the page's minimum / maximum: unsigned bytewise
 * lexicographic order, a proper prefix smaller (Rust slice Ord); among
 * equal values the smallest row; UINT64_MAX in both for a page without a
 * non-null value.
 *
 * A measure pass sizes every page's payload (sum of len + varint_len(len)
 * over its non-null rows) before anything is written; the call holds one
 * scratch buffer of that many bytes for its duration.
 * Errors: GS_ERR (before any device work) for a NULL required pointer,
 * npages <= 0 or a negative h_rows / h_row_off entry; GS_ERR_FORMAT when an
 * offset decreases inside a page; GS_ERR_CAP when cap_per_page <
 * 16 + ceil(rows/8) + 2 + 32 + payload + payload/6 for any page.  The last
 * two are found by the measure pass: no byte of d_out is written.  A failed
 * call leaves the context usable. */
GsStatus gs_encode_str_pages_dev(
    GsCtx *ctx,
    const int64_t *d_offsets,  /* Arrow varbinary, as gs_decode_str leaves it */
    const uint8_t *d_bytes,
    const uint8_t *d_valid,    /* 1 B/row, NULL = all valid */
    const int64_t *h_row_off, const int32_t *h_rows, int32_t npages,
    uint8_t *d_out, int64_t cap_per_page,
    GsPageInfo *h_info);       /* [npages] */

/* ---- compaction merge (BASELINE config #5) ----
 * k overlapping L0 column-group streams per series -> one merged, deduped
 * (ts, value, validity) stream per series (tskv/src/compaction/compact.rs:
 * 271-404, comapcting_block_meta_group.rs:52-208; dedup rule
 * reader/batch_builder.rs:106-155).  sets[f] (f = 0 oldest .. nsets-1
 * newest, file_id order) must cover the same series list; d_ts/d_val/
 * d_valid[f] are that stream's decoded columns (from gs_decode).  Outputs
 * are caller device buffers sized >= the sum of input rows;
 * h_out_offsets[nseries+1] receives per-series output row offsets.
 * d_valid (the array or an entry) and d_out_valid may be NULL; a null
 * cell's value is zero bits.  This is the one-column case of
 * gs_compact_merge_fields (below, ncols = 1, elem_size = {8}) and runs the
 * same kernels.  A stream whose timestamps are not strictly increasing
 * within a series fails with GS_ERR_FORMAT; the output buffers are then
 * unspecified. */
GsStatus gs_compact_merge(GsCtx *ctx, GsGroupSet *const *sets, int32_t nsets,
                          const int64_t *const *d_ts,
                          const double *const *d_val,
                          const uint8_t *const *d_valid, int64_t *d_out_ts,
                          double *d_out_val, uint8_t *d_out_valid,
                          int64_t *h_out_offsets, int64_t *out_rows);

/* ---- compaction merge over every field column of a column group ----
 * The reference never compacts one column at a time: a column group is a
 * time column plus all of the table's field columns, and
 * BatchMergeBuilder::take_last_and_merge (tskv/src/reader/
 * batch_builder.rs:132-155) resolves each column independently over the
 * rows that share a timestamp.  Streams, series lists, the merged
 * timestamp stream (sorted union per series), h_out_offsets and out_rows
 * are exactly those of gs_compact_merge; raw sets (gs_raw_set) are
 * accepted like any other set.  The ownership/rank work depends on the
 * timestamps only and runs once for any ncols.
 *
 * Per cell (timestamp, column c): the value comes from the NEWEST stream
 * that contains the timestamp, has column c present and is valid there —
 * a newer null never hides an older valid value.  With no such stream the
 * value slot is all-zero bytes and the validity byte 0.
 *
 * d_val / d_valid are [nsets*ncols] tables indexed f*ncols + c.  A NULL
 * d_val entry means column c is absent from stream f (an older file after
 * ALTER TABLE ADD FIELD has no page for it) and behaves exactly like an
 * all-null column; a NULL d_valid entry (or a NULL d_valid array) means
 * all rows valid.  d_out_val[c] (required) and d_out_valid[c] (entries or
 * the array may be NULL) are caller device buffers sized >= the sum of
 * input rows.
 *
 * Values move as raw bits, elem_size[c] bytes each: 8 for f64/i64/u64, 1
 * for bool — the widths gs_decode writes.  No arithmetic touches a value:
 * NaN payloads, i64 beyond 2^53 and u64 beyond 2^63 come out unchanged.
 *
 * GS_ERR (with a message, before any device work) for ncols outside
 * 1..GS_MAX_MERGE_COLS, an elem_size outside {1, 8}, nsets outside
 * 1..GS_MAX_STREAMS, a NULL required pointer, or mismatched series
 * counts.  An unsorted stream fails as in gs_compact_merge. */
#define GS_MAX_STREAMS 16
#define GS_MAX_MERGE_COLS 32

GsStatus gs_compact_merge_fields(
    GsCtx *ctx, GsGroupSet *const *sets, int32_t nsets,
    int32_t ncols, const int32_t *elem_size,   /* [ncols], each 8 or 1 */
    const int64_t *const *d_ts,                /* [nsets] */
    const void *const *d_val,                  /* [nsets*ncols], index f*ncols+c;
                                                  NULL entry = column c absent in stream f */
    const uint8_t *const *d_valid,             /* same indexing; NULL entry = all rows valid;
                                                  the array itself may be NULL */
    int64_t *d_out_ts,
    void *const *d_out_val,                    /* [ncols] */
    uint8_t *const *d_out_valid,               /* [ncols]; entries or the array may be NULL */
    int64_t *h_out_offsets, int64_t *out_rows);

/* ---- compaction merge of a column group with string fields ----
 * gs_compact_merge_fields plus nstr string columns (the DataType::Utf8
 * fields of a column group, tsm/page.rs:299-325), each in Arrow varbinary
 * layout as gs_decode_str leaves it.  A string column follows the rule of
 * every other column (take_last_and_merge, batch_builder.rs:132-155): the
 * newest stream that contains the timestamp, has the column and is valid
 * there wins; with no such stream the cell is null with length 0.  A
 * stream's column with d_offsets == NULL is absent there and behaves like
 * an all-null column.  The merged column c is written as
 * str_out[c].d_offsets (out_rows + 1 entries; the buffer holds the sum of
 * input rows + 1), d_bytes and, when not NULL, d_valid; the result is what
 * gs_encode_str_pages_dev takes.  Bytes of null input rows are never read.
 *
 * ncols >= 0, nstr >= 0 and 1 <= ncols + nstr <= GS_MAX_MERGE_COLS.  With
 * nstr == 0 the call IS gs_compact_merge_fields (one internal function, so
 * the timestamp rank work runs once for any mix of columns).  d_out_ts,
 * the fixed-width outputs, h_out_offsets and out_rows are as there.
 *
 * GS_ERR as for gs_compact_merge_fields, and for more than 2^28 output
 * rows with a string column (the device scan's limit).  GS_ERR_CAP when a
 * column's total_bytes exceeds its bytes_cap: every str_out[c].total_bytes
 * is filled, so the caller can size the buffers and call again, no d_bytes
 * of any column is written, and everything else is as on success.  While
 * it runs the call holds 8 B per input row (one reference array per
 * stream) and 8 B per output row and string column. */
typedef struct {                /* one stream's string column */
    const int64_t *d_offsets;   /* int64[rows_f + 1]; NULL = column absent in this stream */
    const uint8_t *d_bytes;
    const uint8_t *d_valid;     /* NULL = all valid */
} GsStrColumn;

typedef struct {                /* one merged string column */
    int64_t *d_offsets;         /* int64[sum of input rows + 1] */
    uint8_t *d_bytes;
    int64_t bytes_cap;
    uint8_t *d_valid;           /* may be NULL */
    int64_t total_bytes;        /* out: d_offsets[out_rows] */
} GsStrColumnOut;

GsStatus gs_compact_merge_group(
    GsCtx *ctx, GsGroupSet *const *sets, int32_t nsets,
    int32_t ncols, const int32_t *elem_size,
    const int64_t *const *d_ts, const void *const *d_val,
    const uint8_t *const *d_valid,
    int32_t nstr, const GsStrColumn *str_in,   /* [nsets*nstr], index f*nstr + c */
    int64_t *d_out_ts, void *const *d_out_val, uint8_t *const *d_out_valid,
    GsStrColumnOut *str_out,                   /* [nstr] */
    int64_t *h_out_offsets, int64_t *out_rows);

/* ---- DataFilter over a column group: multi-column predicates ----
 * The reference's DataFilter (tskv/src/reader/filter.rs:91-142) evaluates
 * ONE pushed expression over the whole RecordBatch and filters every
 * projected column with the resulting mask; decode_pages
 * (tsm/reader.rs:494-560) has applied the tombstones before that: ranges
 * that exclude all fields remove the row (time_null_bits, then
 * filter_record_batch), per-column ranges null that column's cells.
 * gs_filter_group is both steps over decoded columns exactly as gs_decode
 * and gs_decode_str leave them (the convention of gs_compact_merge_fields;
 * a raw set, gs_raw_set, works like a page set): one mask from a
 * conjunction of typed predicates over any of the group's columns, and
 * every projected column compacted by that mask, with its validity.
 *
 * Tombstone ranges.  Every range is closed: a row is inside iff
 * min_ts <= ts <= max_ts, which on strictly increasing timestamps is
 * update_nullbits_by_time_range (tsm/reader.rs:634-656).  A list may be
 * unsorted and overlapping; a range with min_ts > max_ts matches nothing.
 * Ranges apply to every group of the set, as in gs_apply_tombstone.
 *
 * Effective validity of cell (r, c) = valid[c][r] AND ts[r] lies in none of
 * column c's ranges.  Predicates and outputs both see the effective
 * validity, never the raw one.
 *
 * Keep rule.  Row r is kept iff ts[r] is in spec->range, ts[r] is in no row
 * tombstone, and every predicate holds.  A comparison on an effectively
 * null cell fails (arrow's comparison with null is null, and
 * filter_record_batch treats null as false).  GS_PRED_IS_NULL and
 * GS_PRED_IS_NOT_NULL test the effective validity and never read the value.
 *
 * Comparisons run in the column's own type, on the constant's raw bits:
 * i64 signed, u64 unsigned, bool as 0/1, so `x >= 2^53 + 1` on an i64
 * column and a u64 bound above 2^63 mean what they say.  f64 compares with
 * the IEEE operators exactly as gs_scan's value predicate does: NaN fails
 * everything but NE, and -0.0 == +0.0; the two entries agree on every
 * input.  Whether arrow 42's comparison kernels order NaN and signed zero
 * the same way is NOT VERIFIED here; no parity with the reference is
 * claimed on those two inputs.
 *
 * Outputs.  Kept rows stay in input order.  h_out_offsets[g] is the output
 * row at which group g's rows start, h_out_offsets[gs_set_groups] ==
 * *out_rows.  A projected cell that is effectively null has all-zero value
 * bytes and validity 0, like gs_compact_merge_fields, whatever its input
 * slot held: the output is bit-comparable.  A projected string column is
 * Arrow varbinary in GsStrColumnOut (d_offsets holds gs_set_rows + 1
 * entries); a null cell has length 0, and bytes of null input rows are
 * never read.  A column with d_out_val == NULL (out == NULL for a string
 * column) only serves predicates.  GS_ERR_CAP when a string column's
 * total_bytes exceeds its bytes_cap: every total_bytes is filled, no
 * d_bytes of any column is written and everything else is as on success
 * (the gs_compact_merge_group protocol: size the buffers, call again).
 *
 * GS_ERR (with a message, before any device work) for ncols + nstr outside
 * 1..GS_MAX_MERGE_COLS, npreds outside 0..GS_MAX_FILTER_PREDS, a ctype
 * other than the four fixed-width types, a predicate whose col is out of
 * range, a comparison op on a string column, an unknown op, a NULL
 * required pointer, or a string column with more than 2^28 rows in the set
 * (the device scan's limit).  A failed call leaves the context usable.
 * gs_scan does not take the two null tests. */
#define GS_MAX_FILTER_PREDS 16
enum { GS_PRED_IS_NULL = 8, GS_PRED_IS_NOT_NULL = 9 }; /* gs_filter_group only */

typedef struct {
    int32_t col;      /* 0..ncols-1 = cols[col]; ncols+s = string column s
                         (IS_NULL / IS_NOT_NULL only) */
    int32_t op;       /* GS_PRED_GT..GS_PRED_BETWEEN, IS_NULL, IS_NOT_NULL */
    uint64_t a_bits;  /* the constant in the COLUMN'S OWN TYPE, raw bits:
                         f64 bits, i64, u64, bool 0/1 */
    uint64_t b_bits;  /* BETWEEN upper bound (closed) */
} GsColPred;

typedef struct {
    uint8_t ctype;                  /* GS_CT_I64 / F64 / BOOL / U64 */
    const void *d_val;              /* 8 B/row, bool 1 B/row */
    const uint8_t *d_valid;         /* NULL = all valid */
    const GsTimeRange *tombstones;  /* host; this column's deleted ranges */
    size_t n_tombstones;
    void *d_out_val;                /* NULL = predicate-only, not projected */
    uint8_t *d_out_valid;           /* may be NULL */
} GsFilterCol;

typedef struct {
    GsStrColumn in;                 /* as gs_decode_str leaves it */
    const GsTimeRange *tombstones;
    size_t n_tombstones;
    GsStrColumnOut *out;            /* NULL = not projected */
} GsFilterStrCol;

typedef struct {
    GsTimeRange range;                    /* closed */
    const GsTimeRange *row_tombstones;    /* all-fields ranges: row removed */
    size_t n_row_tombstones;
    const GsColPred *preds;               /* conjunction; npreds 0 = none */
    int32_t npreds;
} GsFilterSpec;

GsStatus gs_filter_group(GsCtx *ctx, GsGroupSet *set, const int64_t *d_ts,
                         const GsFilterSpec *spec,
                         int32_t ncols, const GsFilterCol *cols,
                         int32_t nstr, const GsFilterStrCol *strs,
                         int64_t *d_out_ts,      /* >= gs_set_rows rows */
                         int64_t *h_out_offsets, /* [gs_set_groups + 1] */
                         int64_t *out_rows);

/* ---- Typed bucket aggregates over a filtered column group ----
 * gs_agg_group evaluates the keep rule of gs_filter_group and reduces the
 * kept, effectively valid cells of any fixed-width column straight into
 * (series, bucket) cells: count, sum, min, max, first and last in the
 * column's own type.  No row output is written; what gs_filter_group would
 * have handed to a host-side aggregation (`max(usage_user), min(usage_idle)
 * WHERE usage_system > 90 AND usage_nice IS NOT NULL GROUP BY time(5m)`,
 * TSBS lastpoint, any aggregate over an i64 counter) stays on the device.
 *
 * Keep rule and validity.  Word for word those of gs_filter_group, on the
 * same GsFilterSpec / GsFilterCol / GsFilterStrCol and through the same
 * code.  d_out_val / d_out_valid / out are ignored; string columns serve
 * predicates only; a raw set (gs_raw_set) works like a page set.
 *
 * Series.  A series is a series-level group of the set (gs_set_series:
 * consecutive column groups of one series_id merged).
 *
 * Buckets.  A row with ts < t0 is in no bucket.  Otherwise
 * b = uint64(ts - t0) / bucket_ns, formed without signed overflow, and
 * b >= n_buckets is in no bucket.  bucket_ns == 0 is one bucket that holds
 * every row, whatever t0.  Rows in no bucket contribute to nothing, d_rows
 * included.
 *
 * Cells.  per_series 1: cell s * n_buckets + b of gs_set_series * n_buckets;
 * per_series 0: cell b of n_buckets, reduced over the series.  Every cell of
 * every requested array is written by the call exactly as defined: the
 * caller pre-fills nothing and the call does not accumulate into the
 * buffers (unlike gs_scan).  An empty cell holds count 0, sum 0 bits, min /
 * max the starting values of the page statistics (INT64_MAX / INT64_MIN,
 * UINT64_MAX / 0, bool 1 / 0, f64 +inf / -inf: gs_scan's -inf convention
 * for max), first / last 0 bits, first_ts INT64_MAX, last_ts INT64_MIN.
 *
 * count is the number of kept rows whose cell is effectively valid; d_rows
 * the number of kept rows (COUNT(*)).  sum is raw bits: f64 for f64, i64 and
 * u64 wrapping modulo 2^64, for bool the number of true cells as u64.
 * Whether DataFusion 27's SUM wraps or errors on integer overflow is NOT
 * VERIFIED here; no parity with the reference is claimed on a sum that
 * overflows.
 *
 * Min and max use strict compares in the column's type, in row order: a
 * NaN changes neither bound, and of +0.0 and -0.0 the extremum keeps the
 * bits of the first in row order (the rule of gs_encode_group_pages_dev's
 * page statistics).  A NaN counts, propagates through sum and can be first
 * / last.  first / last are the values at the smallest / largest kept
 * timestamp with a valid cell, first_ts / last_ts those timestamps.
 *
 * f64 sum.  The bits are the same for two identical calls and for any
 * launch grid; apart from that the summation order is the implementation's.
 * Integer sums are exact modulo 2^64, so order-free.
 *
 * per_series 0.  The same aggregates reduced over the series.  first is the
 * smallest timestamp, among equal timestamps the lowest series index; last
 * the largest timestamp, among equal timestamps the highest series index:
 * row order of the concatenated set.  Min / max ties between +0.0 and -0.0
 * likewise go to the first row of the set.  The (series, bucket) partials
 * are held in device scratch of gs_set_series * n_buckets cells per
 * aggregated column for the time of the call.
 *
 * Precondition.  Timestamps strictly increase inside a series, as decode
 * leaves them.  A violation returns GS_ERR_FORMAT (the gs_compact_merge
 * rule); the output buffers are then unspecified.
 *
 * GS_ERR (with a message, before any device work) for everything
 * gs_filter_group refuses, naggs outside 1..GS_MAX_MERGE_COLS, an
 * outs[i].col outside 0..ncols-1, n_buckets < 1, bucket_ns < 0,
 * bucket_ns == 0 with n_buckets != 1, more than 2^31 - 1 cells, or a NULL
 * required pointer.  A failed call leaves the context usable.  A set with
 * zero rows succeeds and writes the empty-cell values. */
typedef struct {
    int64_t t0;          /* bucket origin */
    int64_t bucket_ns;   /* >= 1; 0 = one bucket holding every row
                            (n_buckets must be 1) */
    int32_t n_buckets;   /* >= 1 */
    int32_t per_series;  /* 1: cells [gs_set_series * n_buckets], index
                            s * n_buckets + b
                            0: cells [n_buckets], reduced over the series */
} GsAggSpec;

typedef struct {          /* one aggregated column; every array is device
                             memory of 8 B per cell, NULL = not wanted */
    int32_t col;          /* index into cols[] (fixed-width columns only) */
    int64_t *d_count;     /* kept rows whose cell is effectively valid */
    uint64_t *d_sum;      /* raw bits: f64 -> f64; i64 -> i64 and u64 -> u64,
                             both wrapping; bool -> u64 number of true cells */
    uint64_t *d_min, *d_max;     /* raw bits in the column's type, bool 0/1 */
    uint64_t *d_first, *d_last;  /* value at the smallest / largest kept
                                    timestamp with a valid cell */
    int64_t *d_first_ts, *d_last_ts;
} GsAggOut;

GsStatus gs_agg_group(GsCtx *ctx, GsGroupSet *set, const int64_t *d_ts,
                      const GsFilterSpec *filter,
                      int32_t ncols, const GsFilterCol *cols,
                      int32_t nstr, const GsFilterStrCol *strs,
                      const GsAggSpec *agg, int32_t naggs,
                      const GsAggOut *outs,
                      int64_t *d_rows /* [cells] kept rows per cell
                                         (COUNT(*)); may be NULL */);

/* ---- Arrow C Data Interface export (decode output as
 * ArrowArray so the Rust shim reconstitutes RecordBatches zero-copy from
 * the shim's side).  GsArrowArray is layout-identical to `struct
 * ArrowArray` of the Arrow C data interface; for primitive columns
 * buffers = {validity bitmap or NULL, data}. */
typedef struct GsArrowArray {
    int64_t length;
    int64_t null_count;
    int64_t offset;
    int64_t n_buffers;
    int64_t n_children;
    const void **buffers;
    struct GsArrowArray **children;
    struct GsArrowArray *dictionary;
    void (*release)(struct GsArrowArray *);
    void *private_data;
} GsArrowArray;

/* Copy one group's rows of a decoded device column into a freshly
 * allocated host ArrowArray (validity bytes packed LSB-first into the
 * arrow bitmap; d_valid NULL => no validity buffer, null_count 0).
 * elem_size: 8 for i64/f64/u64, 1 for bool (exported as byte values —
 * the shim repacks to arrow bool bits if needed).  Caller releases via
 * out->release(out). */
GsStatus gs_export_group_column(GsCtx *ctx, GsGroupSet *set, int64_t group,
                                const void *d_col, int32_t elem_size,
                                const uint8_t *d_valid, GsArrowArray *out);

#ifdef __cplusplus
}
#endif
#endif /* CNOSDB_GS_H */
