/* cnosdb_gs engine: HIP/CDNA4 (gfx950) kernels for the TSM DataBlock
 * decode + predicate-filtered time-range scan + downsampling aggregates,
 * and the C-ABI host orchestration around them.
 *
 * Decode semantics mirror, bit-exactly:
 *   timestamp / integer / simple8b / boolean pages: see gs_int_dec.h
 *   tskv/src/tsm/codec/float.rs:351-606       (Gorilla, sentinel-terminated)
 *   tskv/src/tsm/reader.rs:494-560,634-656    (decode_pages + tombstone)
 *
 * MI355X mapping (this path is HBM-bandwidth-bound integer/bit work — no
 * MFMA): page-level parallelism across the 256 CUs; inherently sequential
 * bitstreams (Gorilla) decode one page per thread with many pages in
 * flight; closed-form encodings (RLE) decode one workgroup per page fully
 * parallel.  All launches are grid-strided and sized per Guideline 11.
 */
#include <hip/hip_runtime.h>
#include "../../include/cnosdb_gs.h"
#include "gs_internal.h"
#include "gs_gorilla.h"
#include "gs_tsm_enc.h"
#include "gs_str_dec.h"
#include "gs_int_dec.h"
#include "gs_str_enc.h"
#include "gs_filter.h"
#include "gs_agg.h"

/* hipError_t returns are checked with HIP_TRY on every path that can fail
 * user-visibly; cleanup paths (hipFree/hipEventDestroy in destructors) and
 * async enqueues deliberately drop the return — every enqueue is followed
 * by a checked hipStreamSynchronize on the same stream, which surfaces any
 * deferred error.  Silence the nodiscard noise for those. */
#pragma clang diagnostic ignored "-Wunused-value"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <string>

/* ------------------------------------------------------------- error glue */
static thread_local char g_err[512] = "";
static GsStatus fail(GsStatus s, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return s;
}
extern "C" const char *gs_last_error(void) { return g_err; }

#define HIP_TRY(expr)                                                          \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) {                                                \
            snprintf(g_err, sizeof(g_err), "%s: %s", #expr,                    \
                     hipGetErrorString(_e));                                   \
            return GS_ERR;                                                     \
        }                                                                      \
    } while (0)

#define HIP_TRY_NULL(expr)                                                     \
    do {                                                                       \
        hipError_t _e = (expr);                                                \
        if (_e != hipSuccess) {                                                \
            snprintf(g_err, sizeof(g_err), "%s: %s", #expr,                    \
                     hipGetErrorString(_e));                                   \
            return nullptr;                                                    \
        }                                                                      \
    } while (0)

/* ------------------------------------------------------------ device utils */

__device__ __forceinline__ uint64_t dev_be64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}
__device__ __forceinline__ int dev_bit(const uint8_t *bs, uint32_t i) {
    return (bs[i >> 3] >> (i & 7)) & 1;
}
__device__ __forceinline__ uint64_t dev_rotl64(uint64_t x, unsigned c) {
    c &= 63;
    return c ? (x << c) | (x >> (64 - c)) : x;
}

/* error codes accumulated into d_err */
#define DERR_FORMAT 1u
#define DERR_SHORT 2u
static_assert(STR_ERR_FORMAT == DERR_FORMAT && STR_ERR_SHORT == DERR_SHORT,
              "k_str_decode raises str_page_decode's verdict as is");
static_assert(INT_ERR_FORMAT == DERR_FORMAT && INT_ERR_SHORT == DERR_SHORT,
              "the int and bool kernels raise gs_int_dec.h's verdicts as is");
#define DERR_NONMONO 4u /* a CRC-valid but non-monotonic time
                           page would silently mis-select rows via the
                           binary-search span/tombstone kernels; fail
                           loudly instead (the reference's row-wise
                           filtering cannot mis-select) */
static_assert(INT_ERR_NONMONO == DERR_NONMONO, "as above");
/* raised by the encode kernels only, read by enc_dev_status */
#define DERR_ENC_SENTINEL 8u /* Gorilla sentinel as an input value */
#define DERR_ENC_NULL 16u    /* null row in a ts/i64 page */

/* ---------------------------------------------------------------- kernels */

/* Universal sequential decoder for int64-family pages (TIME/I64/U64):
 * one thread per page, grid-strided (int_page_decode, gs_int_dec.h). */
__global__ void k_seq_i64(const uint8_t *__restrict__ blob,
                          const DevPage *__restrict__ pages, int npages,
                          int64_t *__restrict__ out,
                          uint8_t *__restrict__ valid,
                          unsigned *__restrict__ err) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npages;
         p += gridDim.x * blockDim.x) {
        const DevPage pg = pages[p];
        const unsigned e = int_page_decode(
            blob + pg.data_off, pg.data_len, pg.enc, pg.ctype == GS_CT_TIME,
            blob + pg.bitset_off, pg.all_valid, pg.nrows, out + pg.row_off,
            valid ? valid + pg.row_off : nullptr);
        if (e) atomicOr(err, e);
    }
}

#define GS_RING 16
#define GS_GOR_BLOCK 256 /* 4 waves; RING 8/16/32 x block 128/256 swept: 16/256 optimal */

/* --- Gorilla chunked decode (see DevGorChunk in gs_internal.h; the stream
 * format and the window parser live in gs_gorilla.h) ---
 * k_gor_sync: one-time upload pre-pass.  One thread walks each multi-chunk
 * all-valid Gorilla page with the same window parser as decode (no value
 * stores) and records the parser state every chunk_rows values, so decode
 * can start mid-stream.  Errors are NOT raised here: a truncated or
 * early-sentinel page poisons its unrecorded chunks (bitpos past the
 * stream end), and the decode of that chunk raises DERR_SHORT exactly
 * where a page-sequential decode would have — same error surface,
 * surfaced at decode/scan time like the reference's decode errors. */
__global__ void k_gor_sync(const uint8_t *__restrict__ blob,
                           const DevPage *__restrict__ pages, int npages,
                           const int32_t *__restrict__ chunk_base,
                           DevGorChunk *__restrict__ chunks,
                           uint32_t chunk_rows) {
    for (int pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npages;
         pi += gridDim.x * blockDim.x) {
        DevPage pg = pages[pi];
        int cb = chunk_base[pi];
        int nch = chunk_base[pi + 1] - cb;
        if (nch <= 1) continue; /* single chunk: decode reads the header */
        int next_k = 1;
        /* value-initialised, here and in the three kernels below: left
           indeterminate on the short-page path, the state cost registers
           and k_gor_sync_null recorded wrong tables on a set of 625,000
           pages ("One parser for the four cold kernels") */
        GorChunkState st{};
        uint32_t r = 1; /* header value = row 0 */
        bool ok = false;
        if (gor_start(st, blob + pg.data_off, pg.data_len)) {
            ok = true;
            for (;;) {
                if (r == uint32_t(next_k) * chunk_rows) {
                    if (gor_used_bits(st) > st.total_bits) {
                        ok = false;
                        break;
                    }
                    gor_record(st, chunks[cb + next_k]);
                    /* the previous chunk's whole range is now known
                       decodable: the filtered kernel may stop it early */
                    chunks[cb + next_k - 1].flags = GORF_SAFE_STOP;
                    next_k++;
                    if (next_k == nch) break; /* tail chunk parses itself */
                }
                if (st.nb < 64) gor_topup(st);
                if (st.over) { ok = false; break; }
                /* sentinel before the last sync point: rows missing */
                if (gor_parse(st) && st.val == GORILLA_SENTINEL) {
                    ok = false;
                    break;
                }
                r++;
            }
        }
        if (!ok) /* poison unrecorded chunks -> DERR_SHORT at decode */
            for (int k = next_k; k < nch; k++)
                gor_poison(chunks[cb + k], pg.data_len);
    }
}

/* One wave flushes its LDS ring: every lane posts {element offset into
 * out, staged count} of its run, then the wave stores all 64 runs with
 * chunk-contiguous coalesced stores.  4 source lanes per store instruction:
 * lane = (sq:2, idx:4), sq picks the source sub-lane, idx the ring slot,
 * reads batched 4 deep before their stores.  An offset, not a pointer: a
 * pointer that travels through LDS loses its address space and the stores
 * become flat (see k_gor_chunks_filtered, which keeps its own copy of this
 * loop next to its output cursor). */
__device__ __forceinline__ void gor_ring_flush(double (*rslot)[64 + 1],
                                               uint64_t (*fd)[2], int lane,
                                               double *__restrict__ out,
                                               uint64_t o_off, int rfill) {
    const int f_idx = lane & (GS_RING - 1);
    const int f_sq = lane / GS_RING;
    fd[lane][0] = o_off;
    fd[lane][1] = uint64_t(rfill);
    __builtin_amdgcn_wave_barrier();
    constexpr int SRCP = 64 / GS_RING; /* sources per store */
    for (int src0 = 0; src0 < 64; src0 += SRCP * 4) {
        double vbuf[4];
        uint64_t ob[4];
        int cnt[4];
        for (int t = 0; t < 4; t++) {
            int src = src0 + f_sq + t * SRCP;
            vbuf[t] = rslot[f_idx][src];
            ob[t] = fd[src][0];
            cnt[t] = int(fd[src][1]);
        }
        for (int t = 0; t < 4; t++)
            if (f_idx < cnt[t]) out[ob[t] + uint64_t(f_idx)] = vbuf[t];
    }
}

/* Chunk-parallel Gorilla decode with LDS-staged output: each lane decodes
 * one chunk, staging GS_RING values in LDS; the wave flushes cooperatively
 * with chunk-contiguous coalesced stores.  The direct per-lane 8-B stores
 * of the naive version touch 64 distinct cache lines per wave-store and
 * were measured address-bound (profiles/: storeonly 11.8 ms vs lds-staged
 * ~3 ms for the same bytes).  Lanes run in lockstep (one value per
 * iteration), so rings fill together; lanes whose chunk ended keep
 * cooperating in flushes until all are done.  Chunks are page-major in
 * the table, so a wave's lanes hold NEIGHBORING regions of one page. */
__global__ void k_gor_chunks(const uint8_t *__restrict__ blob,
                             const DevGorChunk *__restrict__ chunks,
                             int nchunks, double *__restrict__ out,
                             unsigned *__restrict__ err) {
    __shared__ double ring[GS_GOR_BLOCK / 64][GS_RING][64 + 1];
    __shared__ uint64_t fdesc[GS_GOR_BLOCK / 64][64][2];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    auto rslot = ring[wv];
    int stride = gridDim.x * blockDim.x;
    int base_id = blockIdx.x * blockDim.x + threadIdx.x;
    int rounds = (nchunks + stride - 1) / stride;
    for (int rd = 0; rd < rounds; rd++) {
        int ci = base_id + rd * stride;
        bool have = ci < nchunks;
        /* branch-free prologue: clamp to chunk 0 so every load issues
           unconditionally (see k_gor_chunks_filtered) */
        DevGorChunk ch = chunks[have ? ci : 0];
        uint32_t r = ch.row0;
        uint32_t end = ch.row0 + ch.cnt;
        if (ch.cnt == 0) have = false; /* the one chunk of a zero-row page */
        GorChunkState st{};
        gor_position(st, blob, ch);
        int rfill = 0;
        bool done = !have;
        if (!have) { r = 0; end = 0; }
        if (have && st.bad) { atomicOr(err, DERR_SHORT); done = true; }
        auto flush = [&]() {
            gor_ring_flush(rslot, fdesc[wv], lane, out,
                           uint64_t(ch.row_off + int64_t(r) - rfill), rfill);
            rfill = 0;
        };
        if (!done && ch.row0 == 0 && r < end) { /* header value = row 0 */
            rslot[rfill][lane] = __longlong_as_double((long long)st.val);
            rfill++;
            r++;
        }
        unsigned it = 1; /* header stage counts toward the first cadence */
        while (!__all(done)) {
            if (!done) {
                if (st.nb < 64) gor_topup(st);
                if (st.over) { atomicOr(err, DERR_SHORT); done = true; }
            }
            if (!done) {
                bool stg = true;
                if (gor_parse(st) && st.val == GORILLA_SENTINEL) {
                    done = true;
                    stg = false;
                    if (gor_used_bits(st) > st.total_bits)
                        atomicOr(err, DERR_SHORT);
                }
                if (stg && r < end) {
                    rslot[rfill][lane] =
                        __longlong_as_double((long long)st.val);
                    rfill++;
                    r++;
                    /* non-last chunk: all rows produced, stop; the last
                       chunk keeps parsing to the sentinel like a page-
                       sequential decode (a missing sentinel is an error) */
                    if (r == end && !ch.last) {
                        done = true;
                        if (gor_used_bits(st) > st.total_bits)
                            atomicOr(err, DERR_SHORT);
                    }
                }
            }
            /* uniform cadence: <=1 staged/iteration, so a flush every
               GS_RING iterations can never overflow the ring — no ballot,
               no divergent branch */
            if ((++it & (GS_RING - 1)) == 0) flush();
        }
        flush();
        if (have && r < end) atomicOr(err, DERR_SHORT);
    }
}

/* --- Gorilla chunked decode for NULL-carrying pages (PC_GORN) ---
 * The encoded stream holds only non-null values, scattered to set bits of
 * the validity bitset (tsm/reader.rs:763-825 / float.rs decode via
 * bitset-driven builder).  The parser state is pipelined ONE VALUE AHEAD:
 * `val` always holds the value pending for the next set-bit row, so a
 * chunk boundary at an arbitrary row needs only (bitpos, pending val,
 * window).  The page header's first f64 is the initial pending value.
 * Chunks are row-ranges; null rows stage 0.0 through the same LDS ring
 * (arrow append_null semantics); validity BYTES are produced separately
 * by k_valid_expand (coalesced), not by this kernel. */
__global__ void k_gor_sync_null(const uint8_t *__restrict__ blob,
                                const DevPage *__restrict__ pages, int npages,
                                const int32_t *__restrict__ chunk_base,
                                DevGorChunk *__restrict__ chunks,
                                uint32_t chunk_rows) {
    for (int pi = blockIdx.x * blockDim.x + threadIdx.x; pi < npages;
         pi += gridDim.x * blockDim.x) {
        DevPage pg = pages[pi];
        int cb = chunk_base[pi];
        int nch = chunk_base[pi + 1] - cb;
        if (nch <= 1) continue;
        const uint8_t *bs = blob + pg.bitset_off;
        int next_k = 1;
        bool sent_seen = false;
        GorChunkState st{}; /* val: pending for the 1st set row */
        uint32_t r = 0; /* ROW cursor */
        bool ok = false;
        if (gor_start(st, blob + pg.data_off, pg.data_len)) {
            ok = true;
            for (;;) {
                if (r == uint32_t(next_k) * chunk_rows) {
                    if (!sent_seen && gor_used_bits(st) > st.total_bits) {
                        ok = false;
                        break;
                    }
                    DevGorChunk &c = chunks[cb + next_k];
                    gor_record(st, c);
                    c.flags = sent_seen ? GORF_SENT_SEEN : 0;
                    next_k++;
                    if (next_k == nch) break;
                    if (sent_seen) continue; /* tail: just mark chunks */
                }
                if (sent_seen) { r++; continue; } /* walk rows to boundary */
                if (st.nb < 64) gor_topup(st);
                if (st.over) { ok = false; break; }
                /* a set row consumes the pending value: parse the next one */
                if (dev_bit(bs, r)) {
                    if (gor_parse(st) && st.val == GORILLA_SENTINEL) {
                        if (gor_used_bits(st) > st.total_bits) {
                            ok = false;
                            break;
                        }
                        sent_seen = true;
                    }
                }
                r++;
            }
        }
        if (!ok) /* poison unrecorded chunks -> DERR_SHORT at decode */
            for (int k = next_k; k < nch; k++)
                gor_poison(chunks[cb + k], pg.data_len);
    }
}

/* Chunk-parallel decode of null-carrying Gorilla pages: per iteration one
 * ROW is staged (parsed pending value for set bits, 0.0 for nulls) and,
 * when the row consumed a value, the next value is parsed ahead.  Same
 * LDS ring/flush as k_gor_chunks. */
__global__ void k_gor_chunks_null(const uint8_t *__restrict__ blob,
                                  const DevGorChunk *__restrict__ chunks,
                                  int nchunks, double *__restrict__ out,
                                  unsigned *__restrict__ err) {
    __shared__ double ring[GS_GOR_BLOCK / 64][GS_RING][64 + 1];
    __shared__ uint64_t fdesc[GS_GOR_BLOCK / 64][64][2];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    auto rslot = ring[wv];
    int stride = gridDim.x * blockDim.x;
    int base_id = blockIdx.x * blockDim.x + threadIdx.x;
    int rounds = (nchunks + stride - 1) / stride;
    for (int rd = 0; rd < rounds; rd++) {
        int ci = base_id + rd * stride;
        bool have = ci < nchunks;
        DevGorChunk ch = chunks[have ? ci : 0];
        const uint8_t *bs = blob + ch.bitset_off;
        uint32_t r = ch.row0;
        /* per-8-row bitset byte, prefetched one ahead like the stream
           refills (measured neutral: the kernel is ~72% memory-parked
           with or without it — the stall is elsewhere, see DESIGN.md
           round-3 notes).  Byte loads are always aligned (the 8-B word
           variant misread flakily at high blob offsets); the +1 read
           tops out one byte past the bitset into the page's own data. */
        uint32_t bb_idx = ch.row0 >> 3;
        uint32_t bb = bs[bb_idx];
        uint32_t bb_next = bs[bb_idx + 1];
        uint32_t end = ch.row0 + ch.cnt;
        bool sent_seen = (ch.flags & GORF_SENT_SEEN) != 0;
        /* a tail chunk after the sentinel holds nulls only and never
           touches the stream: its state stays zero */
        GorChunkState st{};
        if (!sent_seen) gor_position(st, blob, ch);
        int rfill = 0;
        bool done = !have;
        if (!have) { r = 0; end = 0; }
        if (have && st.bad) { atomicOr(err, DERR_SHORT); done = true; }
        auto parse_one = [&]() { /* updates st / sent_seen */
            if (gor_parse(st) && st.val == GORILLA_SENTINEL) {
                if (gor_used_bits(st) > st.total_bits)
                    atomicOr(err, DERR_SHORT);
                sent_seen = true;
            }
        };
        auto flush = [&]() {
            gor_ring_flush(rslot, fdesc[wv], lane, out,
                           uint64_t(ch.row_off + int64_t(r) - rfill), rfill);
            rfill = 0;
        };
        unsigned it = 0;
        while (!__all(done)) {
            if (!done && !sent_seen) {
                if (st.nb < 64) gor_topup(st);
                if (st.over) { atomicOr(err, DERR_SHORT); done = true; }
            }
            if (!done) {
                if (r < end) {
                    const uint32_t bi = r >> 3;
                    if (bi != bb_idx) {
                        bb = bb_next;
                        bb_idx = bi;
                        bb_next = bs[bi + 1];
                    }
                    const int bit = int((bb >> (r & 7)) & 1);
                    uint64_t sbits = 0;
                    bool hole = false; /* set row after the sentinel */
                    if (bit) {
                        if (sent_seen) {
                            atomicOr(err, DERR_SHORT);
                            done = true;
                            hole = true;
                        } else {
                            sbits = st.val;
                        }
                    }
                    if (!hole) {
                        rslot[rfill][lane] =
                            __longlong_as_double((long long)sbits);
                        rfill++;
                        r++;
                        if (bit && !sent_seen) parse_one();
                        if (r == end) {
                            if (!ch.last) {
                                done = true;
                                if (!sent_seen &&
                                    gor_used_bits(st) > st.total_bits)
                                    atomicOr(err, DERR_SHORT);
                            }
                            /* last chunk: keep draining to the sentinel */
                        }
                    }
                } else { /* last chunk drain: parse to the sentinel */
                    if (sent_seen) done = true;
                    else parse_one();
                }
            }
            if ((++it & (GS_RING - 1)) == 0) flush();
        }
        flush();
        if (have && r < end) atomicOr(err, DERR_SHORT);
    }
}

/* validity bytes, decoupled from the decode kernels (coalesced):
 * k_valid_fill: vd=1 over all-valid pages; k_valid_expand: vd=bitset. */
__global__ void k_valid_fill(const DevPage *__restrict__ pages, int npages,
                             uint8_t *__restrict__ valid) {
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        DevPage pg = pages[p];
        uint8_t *vd = valid + pg.row_off;
        for (uint32_t r = threadIdx.x; r < pg.nrows; r += blockDim.x)
            vd[r] = 1;
    }
}

__global__ void k_valid_expand(const uint8_t *__restrict__ blob,
                               const DevPage *__restrict__ pages, int npages,
                               uint8_t *__restrict__ valid) {
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        DevPage pg = pages[p];
        const uint8_t *bs = blob + pg.bitset_off;
        uint8_t *vd = valid + pg.row_off;
        const uint32_t nfull = pg.nrows >> 3; /* whole bytes -> u64 writes */
        for (uint32_t b = threadIdx.x; b < nfull; b += blockDim.x) {
            uint64_t ex = 0;
            uint8_t byte = bs[b];
            for (int k = 0; k < 8; k++)
                ex |= uint64_t((byte >> k) & 1) << (8 * k);
            __builtin_memcpy(vd + (size_t(b) << 3), &ex, 8);
        }
        for (uint32_t r = nfull * 8 + threadIdx.x; r < pg.nrows;
             r += blockDim.x)
            vd[r] = uint8_t(dev_bit(bs, r));
    }
}

__global__ void k_seq_f64(const uint8_t *__restrict__ blob,
                          const DevPage *__restrict__ pages, int npages,
                          double *__restrict__ out,
                          uint8_t *__restrict__ valid,
                          unsigned *__restrict__ err) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npages;
         p += gridDim.x * blockDim.x) {
        DevPage pg = pages[p];
        const uint8_t *data = blob + pg.data_off;
        const uint8_t *bs = blob + pg.bitset_off;
        double *o = out + pg.row_off;
        uint8_t *vd = valid ? valid + pg.row_off : nullptr;
        uint32_t n = pg.nrows;

        if (pg.data_len == 0) {
            for (uint32_t r = 0; r < n; r++) { o[r] = 0.0; if (vd) vd[r] = 0; }
            continue;
        }
        uint8_t enc = pg.enc;
        if (enc == GS_ENC_NULL) {
            const uint8_t *q = data + 1;
            uint32_t avail = (pg.data_len - 1) / 8, used = 0;
            for (uint32_t r = 0; r < n; r++) {
                int v = pg.all_valid ? 1 : dev_bit(bs, r);
                if (v && used < avail) {
                    uint64_t u = dev_be64(q + 8ull * used); used++;
                    o[r] = __longlong_as_double(int64_t(u));
                } else { o[r] = 0.0; v = 0; }
                if (vd) vd[r] = uint8_t(v);
            }
            continue;
        }
        if (enc != GS_ENC_GORILLA) { atomicOr(err, DERR_FORMAT); continue; }
        /* Only streams too short to hold the header value arrive here:
           this kernel runs on F64 slots alone, and gs_groups_upload files
           every F64 Gorilla page with data_len >= 10 under PC_GOR or
           PC_GORN (the chunked kernels), whatever its validity. */
        atomicOr(err, DERR_SHORT);
    }
}

/* bool pages: one thread per page (bool_page_decode, gs_int_dec.h) */
__global__ void k_seq_bool(const uint8_t *__restrict__ blob,
                           const DevPage *__restrict__ pages, int npages,
                           uint8_t *__restrict__ out,
                           uint8_t *__restrict__ valid,
                           unsigned *__restrict__ err) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npages;
         p += gridDim.x * blockDim.x) {
        const DevPage pg = pages[p];
        const unsigned e = bool_page_decode(
            blob + pg.data_off, pg.data_len, pg.enc, blob + pg.bitset_off,
            pg.all_valid, pg.nrows, out + pg.row_off,
            valid ? valid + pg.row_off : nullptr);
        if (e) atomicOr(err, e);
    }
}

/* Closed-form parallel RLE decode (all-valid pages): value[r] =
 * first + r*delta — one workgroup per page, coalesced 8-B stores.
 * (timestamp.rs:226-259 / integer.rs:186-214 semantics.) */
__global__ void k_rle_par(const uint8_t *__restrict__ blob,
                          const DevPage *__restrict__ pages, int npages,
                          int64_t *__restrict__ out,
                          uint8_t *__restrict__ valid,
                          unsigned *__restrict__ err) {
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        DevPage pg = pages[p];
        /* every thread parses the tiny header redundantly (no sync needed) */
        const IntHeader h =
            int_page_header(blob + pg.data_off, pg.data_len, pg.enc);
        const unsigned e = h.verdict | int_rle_nonmono(h, pg.nrows);
        if (e && threadIdx.x == 0) atomicOr(err, e);
        if (h.verdict) continue;
        const int64_t first = h.first, delta = h.rle_delta;
        int64_t *o = out + pg.row_off;
        uint8_t *vd = valid ? valid + pg.row_off : nullptr;
        for (uint32_t r = threadIdx.x; r < pg.nrows; r += blockDim.x) {
            o[r] = int64_t(uint64_t(first) + uint64_t(r) * uint64_t(delta));
            if (vd) vd[r] = 1;
        }
    }
}

/* Block-parallel simple8b delta decode (all-valid DeltaTs/Delta pages,
 * sub-tag 1; timestamp.rs:261-299 / integer.rs:216-248): one workgroup
 * per page.  Words are fixed 8-byte units, so the block scans per-word
 * (value count, delta sum) pairs with a carry, then each thread unpacks
 * its word directly to the right output positions — the delta prefix-sum
 * that is sequential in the reference becomes a block scan. */
__global__ void k_s8b_par(const uint8_t *__restrict__ blob,
                          const DevPage *__restrict__ pages, int npages,
                          int64_t *__restrict__ out,
                          uint8_t *__restrict__ valid,
                          unsigned *__restrict__ err) {
    __shared__ uint32_t scnt[256];
    __shared__ uint64_t ssum[256];
    __shared__ uint64_t carry[2]; /* [0]=value offset, [1]=delta prefix */
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        DevPage pg = pages[p];
        const IntHeader h =
            int_page_header(blob + pg.data_off, pg.data_len, pg.enc);
        if (h.verdict) {
            if (threadIdx.x == 0) atomicOr(err, h.verdict);
            continue;
        }
        const bool is_ts = h.is_ts;
        const uint64_t scaler = h.scaler;
        const int64_t first = h.first;
        const uint8_t *words = h.payload;
        uint32_t nwords = h.payload_len / 8;
        int64_t *o = out + pg.row_off;
        uint8_t *vd = valid ? valid + pg.row_off : nullptr;
        uint32_t n = pg.nrows;
        if (threadIdx.x == 0) {
            if (n > 0) o[0] = first;
            carry[0] = 1; /* first value occupies row 0 */
            carry[1] = 0;
        }
        if (vd)
            for (uint32_t r = threadIdx.x; r < n; r += blockDim.x) vd[r] = 1;
        __syncthreads();
        for (uint32_t tile = 0; tile < nwords; tile += blockDim.x) {
            uint32_t wi = tile + threadIdx.x;
            uint64_t w = 0;
            uint32_t cnt = 0;
            uint64_t dsum = 0;
            unsigned bits = 0;
            uint64_t mask = 0;
            if (wi < nwords) {
                w = dev_be64(words + 8ull * wi);
                int_s8b_word(w, cnt, bits, mask);
                if (bits == 0) {
                    /* runs of "1": delta sum = cnt (x scaler for ts,
                       zigzag-decoded 1 -> -1 for i64) */
                    dsum = is_ts ? uint64_t(cnt) * scaler
                                 : uint64_t(int64_t(-1)) * cnt;
                } else {
                    for (uint32_t k = 0; k < cnt; k++) {
                        uint64_t d = int_s8b_get(w, k, bits, mask);
                        dsum += is_ts ? d * scaler : uint64_t(int_zzdec(d));
                    }
                }
            }
            /* block exclusive scan of (cnt, dsum) */
            scnt[threadIdx.x] = cnt;
            ssum[threadIdx.x] = dsum;
            __syncthreads();
            for (int off = 1; off < int(blockDim.x); off <<= 1) {
                uint32_t c2 = threadIdx.x >= unsigned(off)
                                  ? scnt[threadIdx.x - off] : 0;
                uint64_t s2 = threadIdx.x >= unsigned(off)
                                  ? ssum[threadIdx.x - off] : 0;
                __syncthreads();
                scnt[threadIdx.x] += c2;
                ssum[threadIdx.x] += s2;
                __syncthreads();
            }
            uint64_t voff = carry[0] +
                            (threadIdx.x ? scnt[threadIdx.x - 1] : 0);
            uint64_t dpre = carry[1] +
                            (threadIdx.x ? ssum[threadIdx.x - 1] : 0);
            if (wi < nwords && cnt) {
                uint64_t acc = uint64_t(first) + dpre;
                if (bits == 0) {
                    uint64_t step = is_ts ? scaler : uint64_t(int64_t(-1));
                    for (uint32_t k = 0; k < cnt && voff + k < n; k++) {
                        acc += step;
                        o[voff + k] = int64_t(acc);
                    }
                } else {
                    int64_t pr = int64_t(acc);
                    for (uint32_t k = 0; k < cnt; k++) {
                        uint64_t d = int_s8b_get(w, k, bits, mask);
                        acc += is_ts ? d * scaler : uint64_t(int_zzdec(d));
                        /* ts: i64 wrap of the delta prefix = corrupt page
                           (times must not decrease) */
                        if (is_ts && int64_t(acc) < pr)
                            atomicOr(err, DERR_NONMONO);
                        pr = int64_t(acc);
                        if (voff + k < n) o[voff + k] = int64_t(acc);
                    }
                }
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                carry[0] += scnt[blockDim.x - 1];
                carry[1] += ssum[blockDim.x - 1];
            }
            __syncthreads();
            if (carry[0] >= n) break; /* enough values for every row */
        }
        __syncthreads();
        /* iterator exhaustion: rows past the decoded count are 0
           (k_seq_i64 / Int64Builder skip semantics) */
        uint64_t total = carry[0];
        for (uint64_t r = total + threadIdx.x; r < n; r += blockDim.x)
            o[r] = 0;
        __syncthreads();
    }
}

/* Null-encoded (raw BE) all-valid pages: one workgroup per page, fully
 * coalesced byteswap copy (ts_without_compress_decode_to_array,
 * timestamp.rs:301-323; uncompressed ts carries NO deltas under Null).
 * Works for i64/u64/f64 alike (bit pattern passthrough). */
__global__ void k_raw_par(const uint8_t *__restrict__ blob,
                          const DevPage *__restrict__ pages, int npages,
                          int64_t *__restrict__ out,
                          uint8_t *__restrict__ valid,
                          unsigned *__restrict__ err) {
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        DevPage pg = pages[p];
        const uint8_t *q = blob + pg.data_off + 1;
        uint32_t avail = (pg.data_len - 1) / 8;
        int64_t *o = out + pg.row_off;
        uint8_t *vd = valid ? valid + pg.row_off : nullptr;
        uint32_t n = pg.nrows;
        const bool ck_ts = pg.ctype == GS_CT_TIME;
        for (uint32_t r = threadIdx.x; r < n; r += blockDim.x) {
            int64_t x = (r < avail) ? int64_t(dev_be64(q + 8ull * r)) : 0;
            /* absolute (Null-encoded) time pages may be unsorted: the
               previous input word is an L1 hit */
            if (ck_ts && r > 0 && r < avail &&
                x < int64_t(dev_be64(q + 8ull * (r - 1))))
                atomicOr(err, DERR_NONMONO);
            o[r] = x;
            if (vd) vd[r] = 1;
        }
    }
}

/* BitPack bool pages, all-valid: parallel bit extract (boolean.rs:79-110;
 * MSB-first bits after the varint count) */
__global__ void k_bool_par(const uint8_t *__restrict__ blob,
                           const DevPage *__restrict__ pages, int npages,
                           uint8_t *__restrict__ out,
                           uint8_t *__restrict__ valid,
                           unsigned *__restrict__ err) {
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        DevPage pg = pages[p];
        const BoolHeader h =
            bool_page_header(blob + pg.data_off, pg.data_len, pg.enc);
        if (h.verdict) {
            if (threadIdx.x == 0) atomicOr(err, h.verdict);
            continue;
        }
        const uint64_t count = h.count; /* capped at the bits present */
        uint8_t *o = out + pg.row_off;
        uint8_t *vd = valid ? valid + pg.row_off : nullptr;
        uint32_t n = pg.nrows;
        if (count < n && threadIdx.x == 0) atomicOr(err, DERR_SHORT);
        for (uint32_t r = threadIdx.x; r < n; r += blockDim.x) {
            o[r] = (r < count) ? bool_bit(h.bits, r) : 0;
            if (vd) vd[r] = 1;
        }
    }
}

/* per-group closed-interval span on the sorted decoded ts
 * (TimeRange semantics, domain.rs:36-44) */
__global__ void k_spans(const DevGroup *__restrict__ groups, int n,
                        const int64_t *__restrict__ ts, int64_t mn, int64_t mx,
                        int64_t *__restrict__ sp_start,
                        int64_t *__restrict__ sp_cnt) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < n;
         g += gridDim.x * blockDim.x) {
        const int64_t *t = ts + groups[g].row_off;
        int64_t nr = groups[g].nrows;
        int64_t lo = 0, hi = nr;
        while (lo < hi) { int64_t m = (lo + hi) >> 1; if (t[m] < mn) lo = m + 1; else hi = m; }
        int64_t s = lo;
        lo = 0; hi = nr;
        while (lo < hi) { int64_t m = (lo + hi) >> 1; if (t[m] <= mx) lo = m + 1; else hi = m; }
        sp_start[g] = s;
        sp_cnt[g] = lo - s;
    }
}

/* tombstone masking (tsm/reader.rs:634-656): clear validity for rows whose
 * ts lies in a deleted closed range.  Block per group. */
__global__ void k_tombstone(const DevGroup *__restrict__ groups, int n,
                            const int64_t *__restrict__ ts,
                            uint8_t *__restrict__ valid,
                            const GsTimeRange *__restrict__ ranges,
                            int nranges) {
    for (int g = blockIdx.x; g < n; g += gridDim.x) {
        const int64_t *t = ts + groups[g].row_off;
        uint8_t *vd = valid + groups[g].row_off;
        int64_t nr = groups[g].nrows;
        for (int q = 0; q < nranges; q++) {
            int64_t mn = ranges[q].min_ts, mx = ranges[q].max_ts;
            int64_t lo = 0, hi = nr;
            while (lo < hi) { int64_t m = (lo + hi) >> 1; if (t[m] < mn) lo = m + 1; else hi = m; }
            int64_t s = lo;
            lo = 0; hi = nr;
            while (lo < hi) { int64_t m = (lo + hi) >> 1; if (t[m] < mx) lo = m + 1; else hi = m; }
            int64_t e = (lo < nr && t[lo] == mx) ? lo + 1 : lo;
            for (int64_t r = s + threadIdx.x; r < e; r += blockDim.x) vd[r] = 0;
        }
    }
}

/* value-predicate mask over the selected span (DataFilter semantics,
 * reader/filter.rs:91-142): mask = validity AND pred(value); per-group
 * selected count by block reduction */
template <typename T>
__device__ __forceinline__ bool dev_pred_t(int op, T a, T b, T x) {
    switch (op) {
    case GS_PRED_GT: return x > a;
    case GS_PRED_GE: return x >= a;
    case GS_PRED_LT: return x < a;
    case GS_PRED_LE: return x <= a;
    case GS_PRED_EQ: return x == a;
    case GS_PRED_NE: return x != a;
    case GS_PRED_BETWEEN: return x >= a && x <= b;
    default: return true;
    }
}

/* vt: 0 = f64, 1 = i64, 2 = u64 (bit-cast slot, unsigned.rs:20-45) — the
 * reference's DataFilter evaluates the pushed expr in the column's own
 * type (reader/filter.rs:91-142) */
__device__ __forceinline__ bool dev_pred(int op, double a, double b,
                                         double x, int vt) {
    if (vt == 1)
        return dev_pred_t<int64_t>(op, int64_t(a), int64_t(b),
                                   __double_as_longlong(x));
    if (vt == 2)
        return dev_pred_t<uint64_t>(op, uint64_t(a), uint64_t(b),
                                    uint64_t(__double_as_longlong(x)));
    return dev_pred_t<double>(op, a, b, x);
}

__global__ void k_vmask(const DevGroup *__restrict__ groups, int n,
                        const double *__restrict__ val,
                        const uint8_t *__restrict__ valid,
                        const int64_t *__restrict__ sp_start,
                        const int64_t *__restrict__ sp_cnt, int op, double a,
                        double b, int vt, uint8_t *__restrict__ mask,
                        int64_t *__restrict__ sel_cnt) {
    __shared__ long long sred[256];
    for (int g = blockIdx.x; g < n; g += gridDim.x) {
        int64_t base = groups[g].row_off + sp_start[g];
        int64_t cnt = sp_cnt[g];
        long long c = 0;
        for (int64_t r = threadIdx.x; r < cnt; r += blockDim.x) {
            bool ok = (!valid || valid[base + r]) &&
                      dev_pred(op, a, b, val[base + r], vt);
            mask[base + r] = ok;
            c += ok;
        }
        sred[threadIdx.x] = c;
        __syncthreads();
        for (int w = blockDim.x >> 1; w > 0; w >>= 1) {
            if (threadIdx.x < unsigned(w)) sred[threadIdx.x] += sred[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) sel_cnt[g] = sred[0];
        __syncthreads();
    }
}

/* masked compaction: block-scan of the mask within the span, gather the
 * selected rows (filter_record_batch's mask-then-gather,
 * reader/filter.rs:130-142) */
__global__ void k_compact_masked(const DevGroup *__restrict__ groups, int n,
                                 const int64_t *__restrict__ ts,
                                 const double *__restrict__ val,
                                 const uint8_t *__restrict__ mask,
                                 const int64_t *__restrict__ sp_start,
                                 const int64_t *__restrict__ sp_cnt,
                                 const int64_t *__restrict__ out_off,
                                 int64_t *__restrict__ out_ts,
                                 double *__restrict__ out_val) {
    __shared__ int32_t sh[256];
    __shared__ int64_t carry;
    for (int g = blockIdx.x; g < n; g += gridDim.x) {
        int64_t base = groups[g].row_off + sp_start[g];
        int64_t cnt = sp_cnt[g];
        int64_t dst = out_off[g];
        if (threadIdx.x == 0) carry = 0;
        __syncthreads();
        for (int64_t tile = 0; tile < cnt; tile += blockDim.x) {
            int64_t r = tile + threadIdx.x;
            int32_t m = (r < cnt) ? mask[base + r] : 0;
            sh[threadIdx.x] = m;
            __syncthreads();
            for (int off = 1; off < int(blockDim.x); off <<= 1) {
                int32_t u = threadIdx.x >= unsigned(off)
                                ? sh[threadIdx.x - off] : 0;
                __syncthreads();
                sh[threadIdx.x] += u;
                __syncthreads();
            }
            if (m) {
                int64_t pos = dst + carry + sh[threadIdx.x] - 1;
                out_ts[pos] = ts[base + r];
                out_val[pos] = val[base + r];
            }
            __syncthreads();
            if (threadIdx.x == 0) carry += sh[blockDim.x - 1];
            __syncthreads();
        }
    }
}

/* compacting copy of the selected span (filter_record_batch semantics,
 * reader/filter.rs:130-142: row filter on time; field nulls travel) */
__global__ void k_compact(const DevGroup *__restrict__ groups, int n,
                          const int64_t *__restrict__ ts,
                          const double *__restrict__ val,
                          const int64_t *__restrict__ sp_start,
                          const int64_t *__restrict__ sp_cnt,
                          const int64_t *__restrict__ out_off,
                          int64_t *__restrict__ out_ts,
                          double *__restrict__ out_val) {
    for (int g = blockIdx.x; g < n; g += gridDim.x) {
        int64_t base = groups[g].row_off + sp_start[g];
        int64_t cnt = sp_cnt[g];
        int64_t dst = out_off[g];
        for (int64_t r = threadIdx.x; r < cnt; r += blockDim.x) {
            out_ts[dst + r] = ts[base + r];
            out_val[dst + r] = val[base + r];
        }
    }
}

/* Fused per-bucket max/sum/count over the selected span, two phases with
 * NO atomics and a deterministic (fixed-tree) float reduction order —
 * BASELINE config #3 requires max exact and sum within stated tolerance,
 * and the reference's DataFusion hash-agg is sequential per partition.
 *
 * Phase 1 (k_agg_partial): block per AGGREGATION GROUP (consecutive
 * page-groups of one series merged at upload — their rows are contiguous
 * and time-ordered, tsm/column_group.rs:55-63).  The decoded ts of a
 * group is sorted, so each bucket's rows form a contiguous range found by
 * binary search (clipped to the scan's closed time range); the block's
 * waves split the bucket list, each wave reduces its bucket's rows with a
 * shuffle tree and writes the (group,bucket) partial.  Every cell is
 * written exactly once — no init needed, no atomics anywhere.
 *
 * Phase 2 (k_agg_merge): one wave per bucket strides the groups, reducing
 * partials in a fixed lane order, and accumulates into the caller's
 * global bucket arrays (sequential across sub-batches => deterministic).
 */
__global__ void k_agg_partial(const DevGroup *__restrict__ groups, int n,
                              const int64_t *__restrict__ ts,
                              const double *__restrict__ val,
                              const uint8_t *__restrict__ valid,
                              int64_t range_lo, int64_t range_hi, int64_t t0,
                              int64_t bucket_ns, int nbuckets,
                              double *__restrict__ pmax,
                              double *__restrict__ psum,
                              long long *__restrict__ pcnt) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nwaves = blockDim.x >> 6;
    /* bucket-boundary row offsets staged in LDS: one cooperative binary
       search per boundary (256 in flight per block) instead of 2 dependent
       searches per (wave,bucket) — the searches were the latency hot spot */
    /* dynamic LDS: sized to nbuckets+1 at launch so occupancy is not
       capped by the worst-case table (32.8 KB static -> 4 blocks/CU even
       for small bucket counts) */
    extern __shared__ __attribute__((aligned(16))) uint32_t soff[];
    constexpr int MAXB = 8192;
    const bool use_lds = nbuckets <= MAXB;
    const int64_t hi_open = (range_hi == INT64_MAX) ? INT64_MAX : range_hi + 1;
    for (int g = blockIdx.x; g < n; g += gridDim.x) {
        const int64_t base = groups[g].row_off;
        const int64_t cnt = groups[g].nrows;
        const int64_t *t = ts + base;
        const double *v = val + base;
        const uint8_t *vd = valid ? valid + base : nullptr;
        if (use_lds) {
            for (int bi = threadIdx.x; bi <= nbuckets; bi += blockDim.x) {
                int64_t bound = t0 + int64_t(bi) * bucket_ns;
                if (bound < range_lo) bound = range_lo;
                if (bound > hi_open) bound = hi_open;
                int64_t lo = 0, hi = cnt;
                while (lo < hi) {
                    int64_t m = (lo + hi) >> 1;
                    if (t[m] < bound) lo = m + 1; else hi = m;
                }
                soff[bi] = uint32_t(lo);
            }
            __syncthreads();
        }
        for (int b = wave; b < nbuckets; b += nwaves) {
            int64_t s, e;
            if (use_lds) {
                s = soff[b];
                e = soff[b + 1];
            } else {
                int64_t blo = t0 + int64_t(b) * bucket_ns;
                int64_t bhi = blo + bucket_ns;
                if (blo < range_lo) blo = range_lo;
                int64_t bhi_cl = (bhi < hi_open) ? bhi : hi_open;
                int64_t lo = 0, hi = cnt;
                while (lo < hi) { int64_t m = (lo + hi) >> 1; if (t[m] < blo) lo = m + 1; else hi = m; }
                s = lo;
                lo = s; hi = cnt;
                while (lo < hi) { int64_t m = (lo + hi) >> 1; if (t[m] < bhi_cl) lo = m + 1; else hi = m; }
                e = lo;
            }
            double mx = -__builtin_inf(), sm = 0.0;
            long long c = 0;
            for (int64_t r = s + lane; r < e; r += 64) {
                if (vd && !vd[r]) continue;
                double x = v[r];
                if (x > mx) mx = x;
                sm += x;
                c++;
            }
            /* wave shuffle tree (fixed order) */
            for (int off = 32; off > 0; off >>= 1) {
                double omx = __shfl_down(mx, off, 64);
                double osm = __shfl_down(sm, off, 64);
                long long oc = __shfl_down(c, off, 64);
                if (omx > mx) mx = omx;
                sm += osm;
                c += oc;
            }
            if (lane == 0) {
                size_t idx = size_t(g) * nbuckets + b;
                pmax[idx] = mx;
                psum[idx] = sm;
                pcnt[idx] = c;
            }
        }
        if (use_lds) __syncthreads();
    }
}

__global__ void k_agg_merge(int ngroups, int nbuckets,
                            const double *__restrict__ pmax,
                            const double *__restrict__ psum,
                            const long long *__restrict__ pcnt,
                            double *__restrict__ gmax,
                            double *__restrict__ gsum,
                            long long *__restrict__ gcnt) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nwaves = blockDim.x >> 6;
    for (int b = blockIdx.x * nwaves + wave; b < nbuckets;
         b += gridDim.x * nwaves) {
        double mx = -__builtin_inf(), sm = 0.0;
        long long c = 0;
        for (int g = lane; g < ngroups; g += 64) {
            size_t idx = size_t(g) * nbuckets + b;
            double omx = pmax[idx];
            if (omx > mx) mx = omx;
            sm += psum[idx];
            c += pcnt[idx];
        }
        for (int off = 32; off > 0; off >>= 1) {
            double omx = __shfl_down(mx, off, 64);
            double osm = __shfl_down(sm, off, 64);
            long long oc = __shfl_down(c, off, 64);
            if (omx > mx) mx = omx;
            sm += osm;
            c += oc;
        }
        if (lane == 0) {
            if (mx > gmax[b]) gmax[b] = mx;
            gsum[b] += sm;
            gcnt[b] += c;
        }
    }
}

/* Fused-path aggregate partial with CLOSED-FORM bucket boundaries, as a
 * SEPARATE pass over the decoded values.  Since the decode kernel learnt
 * to aggregate the rows while it holds them (k_gor_chunks_filtered<true> +
 * k_agg_fixup) this kernel is the fallback: GS_AGG_FUSED=0, buckets below
 * GS_AGG_FUSED_MIN_ROWS rows, or a set whose piece tables do not fit.  It
 * re-reads the 8 B/row the decode just wrote and pays a 64-lane shuffle
 * tree per bucket, which is why it is no longer the default.
 * The fused scan requires every ts page to be RLE (fused_capable), so the
 * compacted output of each page-group is an affine ts sequence
 * (t0sel + i*delta) recorded by k_spans_rle.  Instead of 1 global binary
 * search over out_ts per bucket boundary (the latency + traffic hot spot
 * of k_agg_partial: ~log2(rows) dependent DRAM loads each), boundaries
 * are found by a search over the sgroup's page-group table staged in LDS
 * followed by one division — no out_ts reads at all.  The reduction and
 * partial-cell layout are identical to k_agg_partial (deterministic,
 * every cell written once). */
__global__ void k_agg_partial_rle(const DevGroup *__restrict__ sg, int nsg,
                                  const int32_t *__restrict__ sgfirst,
                                  const int64_t *__restrict__ g_t0sel,
                                  const int64_t *__restrict__ g_delta,
                                  const int64_t *__restrict__ out_off,
                                  const double *__restrict__ val,
                                  int64_t t0, int64_t bucket_ns, int nbuckets,
                                  int max_span,
                                  double *__restrict__ pmax,
                                  double *__restrict__ psum,
                                  long long *__restrict__ pcnt) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int nwaves = blockDim.x >> 6;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int64_t *t0s = (int64_t *)smem;              /* [max_span] */
    int64_t *dlt = t0s + max_span;               /* [max_span] */
    uint32_t *rel = (uint32_t *)(dlt + max_span); /* [max_span+1] */
    uint32_t *soff = rel + max_span + 1;         /* [nbuckets+1] */
    for (int g = blockIdx.x; g < nsg; g += gridDim.x) {
        const int64_t base = sg[g].row_off;
        const int32_t nrows = sg[g].nrows;
        const int gf = sgfirst[g];
        const int span = sgfirst[g + 1] - gf;
        for (int j = threadIdx.x; j < span; j += blockDim.x) {
            rel[j] = uint32_t(out_off[gf + j] - base);
            t0s[j] = g_t0sel[gf + j];
            dlt[j] = g_delta[gf + j];
        }
        if (threadIdx.x == 0) rel[span] = uint32_t(nrows);
        __syncthreads();
        for (int bi = threadIdx.x; bi <= nbuckets; bi += blockDim.x) {
            const int64_t bound = t0 + int64_t(bi) * bucket_ns;
            /* count of selected rows with ts < bound; page-groups of one
               series are time-ordered and non-overlapping */
            int lo = 0, hi = span;
            while (lo < hi) {
                int m = (lo + hi) >> 1;
                if (t0s[m] < bound) lo = m + 1; else hi = m;
            }
            uint32_t off = 0;
            if (lo > 0) {
                const int k = lo - 1;
                const uint32_t cnt = rel[k + 1] - rel[k];
                const int64_t d = dlt[k], b = bound - t0s[k]; /* b > 0 */
                uint32_t w;
                if (d <= 0) {
                    w = cnt; /* constant ts < bound: all rows qualify */
                } else {
                    __int128 q = ((__int128)b + d - 1) / d; /* #i: i*d < b */
                    w = q >= cnt ? cnt : uint32_t(q);
                }
                off = rel[k] + w;
            }
            soff[bi] = off;
        }
        __syncthreads();
        const double *v = val + base;
        /* CONTIGUOUS bucket range per wave, cut at ROW quantiles via the
           soff table: each wave sweeps one monotone row stream of ~equal
           length (HW prefetch friendly + load-balanced even when the
           time range empties the outer buckets).  Empty buckets skip the
           shuffle tree. */
        int b0, b1;
        {
            const uint32_t q0 = uint32_t(int64_t(nrows) * wave / nwaves);
            const uint32_t q1 = uint32_t(int64_t(nrows) * (wave + 1) / nwaves);
            int lo2 = 0, hi2 = nbuckets + 1;
            while (lo2 < hi2) {
                int m = (lo2 + hi2) >> 1;
                if (soff[m] < q0) lo2 = m + 1; else hi2 = m;
            }
            b0 = lo2 < nbuckets ? lo2 : nbuckets;
            hi2 = nbuckets + 1;
            while (lo2 < hi2) {
                int m = (lo2 + hi2) >> 1;
                if (soff[m] < q1) lo2 = m + 1; else hi2 = m;
            }
            b1 = lo2 < nbuckets ? lo2 : nbuckets;
            /* trailing empty buckets (soff hits nrows early) still need
               their partial cells written: stretch the last wave */
            if (wave == nwaves - 1) b1 = nbuckets;
        }
        for (int b = b0; b < b1; b++) {
            const int64_t s = soff[b], e = soff[b + 1];
            size_t idx = size_t(g) * nbuckets + b;
            if (e <= s) {
                if (lane == 0) {
                    pmax[idx] = -__builtin_inf();
                    psum[idx] = 0.0;
                    pcnt[idx] = 0;
                }
                continue;
            }
            /* fused-path rows are all-valid (fused_capable), so the count
               is e-s outright — no count accumulator, no count tree */
            double mx = -__builtin_inf(), sm = 0.0;
            /* 16-B double2 loads: halve the load-instruction traffic of
               the strided 8-B version (the kernel was instruction-bound
               at 3.4 TB/s vs the ~6.3 achievable).  A start row that is
               not 16-B aligned is peeled; the peel goes by the address,
               not the row index, since field f of a multi-field scan
               starts at f*total_rows, odd for an odd total. */
            const int head = int((uintptr_t(v + s) >> 3) & 1);
            if (head && lane == 0) {
                double x = v[s];
                mx = x;
                sm = x;
            }
            const int64_t n2 = (e - s - head) >> 1;
            const double2 *vp = (const double2 *)(v + s + head);
            int64_t q = lane;
            for (; q + 64 < n2; q += 128) { /* 2 loads in flight per iter */
                double2 x0 = vp[q], x1 = vp[q + 64];
                if (x0.x > mx) mx = x0.x;
                if (x0.y > mx) mx = x0.y;
                if (x1.x > mx) mx = x1.x;
                if (x1.y > mx) mx = x1.y;
                sm += (x0.x + x0.y) + (x1.x + x1.y);
            }
            if (q < n2) {
                double2 x = vp[q];
                if (x.x > mx) mx = x.x;
                if (x.y > mx) mx = x.y;
                sm += x.x + x.y;
            }
            if (((e - s - head) & 1) && lane == 63) {
                double x = v[e - 1];
                if (x > mx) mx = x;
                sm += x;
            }
            for (int off2 = 32; off2 > 0; off2 >>= 1) {
                double omx = __shfl_down(mx, off2, 64);
                double osm = __shfl_down(sm, off2, 64);
                if (omx > mx) mx = omx;
                sm += osm;
            }
            if (lane == 0) {
                pmax[idx] = mx;
                psum[idx] = sm;
                pcnt[idx] = e - s;
            }
        }
        __syncthreads();
    }
}

/* --------------------- string column decode (PC_STR) ---------------------
 * codec/string.rs snappy blocks ([7][0x10][snappy raw of varint-prefixed
 * strings]) and uncompressed blocks ([1][u64 BE len][bytes]...).  The
 * snappy bitstream is strictly sequential, so (like Gorilla) parallelism
 * is pages in flight: one thread decompresses one page into its scratch
 * slab, then walks the payload against the validity bitset recording
 * (pos,len) per row; a device scan of the lengths builds the Arrow
 * offsets and a gather packs the bytes.  The decompressor, the walk and
 * the slab accounting are gs_str_dec.h (shared with the host). */

__global__ void k_str_decode(const uint8_t *__restrict__ blob,
                             const DevPage *__restrict__ pages, int n,
                             const int64_t *__restrict__ scr_off,
                             uint8_t *__restrict__ scratch,
                             int64_t *__restrict__ sz,
                             int64_t *__restrict__ pos,
                             uint8_t *__restrict__ valid,
                             unsigned *__restrict__ err) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n;
         p += gridDim.x * blockDim.x) {
        DevPage pg = pages[p];
        const uint8_t *s = blob + pg.data_off;
        const int64_t base = pg.row_off;
        /* the slab at scr_off[p] holds str_slab_size bytes of this page,
           as gs_groups_upload laid it out */
        unsigned e = str_page_decode(
            s, pg.data_len, pg.enc, blob + pg.bitset_off, pg.all_valid,
            pg.nrows, scratch + scr_off[p], scr_off[p], sz + base,
            pos + base, valid ? valid + base : nullptr);
        if (e) atomicOr(err, e);
    }
}

__global__ void k_str_gather(const uint8_t *__restrict__ scratch,
                             const int64_t *__restrict__ pos,
                             const int64_t *__restrict__ sz,
                             const int64_t *__restrict__ off, int64_t rows,
                             uint8_t *__restrict__ out) {
    for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r < rows;
         r += int64_t(gridDim.x) * blockDim.x) {
        const int64_t n2 = sz[r];
        const uint8_t *s = scratch + pos[r];
        uint8_t *d = out + off[r];
        int64_t k = 0;
        for (; k + 8 <= n2; k += 8) { /* word-wide gather */
            uint64_t w;
            __builtin_memcpy(&w, s + k, 8);
            __builtin_memcpy(d + k, &w, 8);
        }
        for (; k < n2; k++) d[k] = s[k];
    }
}

/* ------------------------------------------------- compaction merge (k-way)
 * Config #5: k overlapping L0 column groups per series -> one merged,
 * deduped stream (compact.rs:271-404, comapcting_block_meta_group.rs:
 * 52-208).  Streams are ordered oldest -> newest (file_id order,
 * iterator.rs:488); equal timestamps collapse, per column the newest
 * non-null value wins (batch_builder.rs:106-155).
 *
 * GPU mapping: no loser tree — ranks by binary search.  An element is the
 * row OWNER iff no newer stream contains its ts; the merged position of
 * an owner is the sum over streams of "owners with smaller ts", obtained
 * from per-stream exclusive scans of the owner flags.  Dedup value
 * selection walks streams newest -> oldest at scatter time. */

#define GS_MAX_STREAMS 16

struct CompactArgs {
    const int64_t *ts[GS_MAX_STREAMS];
    const DevGroup *groups[GS_MAX_STREAMS];
    uint8_t *flags[GS_MAX_STREAMS];
    int32_t *prefix[GS_MAX_STREAMS];
    int64_t *counts; /* [nsets][nseries] owner counts */
    int64_t *out_off; /* [nseries] output row offsets */
};

__device__ __forceinline__ bool dev_ts_contains(const int64_t *t, int64_t n,
                                                int64_t x, int64_t *pos) {
    int64_t lo = 0, hi = n;
    while (lo < hi) { int64_t m = (lo + hi) >> 1; if (t[m] < x) lo = m + 1; else hi = m; }
    *pos = lo;
    return lo < n && t[lo] == x;
}

/* block per (set, series): owner flags + per-series owner count.
 *
 * LDS-staged tiled merge (round-2 rework): per 1024-element tile of
 * stream f, the matching window of each NEWER stream is block-loaded
 * into LDS ONCE (coalesced), and every lane searches LDS instead of
 * global memory.  Round-1 searched global per element (log2(n) loads,
 * tolerable only because bisection's top tree levels are L1-shared);
 * three per-lane-probe variants (tiles+gallop, strided+gallop,
 * interpolation) all measured SLOWER than that — staging is the only
 * scheme whose global rank traffic is "each t2 element loaded once".
 * All block-wide loops are uniform (lanes idle within chunks, never
 * diverge across a __syncthreads). */
#define CM_TILE 2048 /* stream-f elements per tile (8 per lane; 1024 and 4096 measured slower) */
#define CM_W 2048    /* LDS window entries (16 KiB) per chunk */

/* Window [wl, wend) of the n2 > 0 sorted rows of t2 that can equal a tile
 * value in [x_lo, x_hi]: thread 0 bisects into wb_sh, the block reads it
 * between two barriers (the second frees wb_sh for the next search). */
__device__ __forceinline__ void cm_window(const int64_t *t2, int64_t n2,
                                          int64_t x_lo, int64_t x_hi,
                                          int64_t *wb_sh, int64_t &wl,
                                          int64_t &wend) {
    if (threadIdx.x == 0) {
        int64_t lo = 0, hi = n2;
        while (lo < hi) {
            int64_t m = (lo + hi) >> 1;
            if (t2[m] < x_lo) lo = m + 1; else hi = m;
        }
        wb_sh[0] = lo;
        int64_t lo2 = lo, hi2 = n2;
        while (lo2 < hi2) {
            int64_t m = (lo2 + hi2) >> 1;
            if (t2[m] <= x_hi) lo2 = m + 1; else hi2 = m;
        }
        wb_sh[1] = lo2;
    }
    __syncthreads();
    wl = wb_sh[0];
    wend = wb_sh[1];
    __syncthreads();
}

/* first i in [0, wcnt] with wts[i] >= x, over the LDS window */
__device__ __forceinline__ int cm_lower_bound(const int64_t *wts, int wcnt,
                                              int64_t x) {
    int lo = 0, hi = wcnt;
    while (lo < hi) {
        int m = (lo + hi) >> 1;
        if (wts[m] < x) lo = m + 1; else hi = m;
    }
    return lo;
}

__global__ void k_cm_flags(CompactArgs a, int nsets, int nseries,
                           unsigned *__restrict__ err) {
    __shared__ int64_t wts[CM_W];
    __shared__ int64_t wb_sh[2];
    __shared__ long long sred[256];
    int f = blockIdx.y;
    for (int s = blockIdx.x; s < nseries; s += gridDim.x) {
        DevGroup g = a.groups[f][s];
        const int64_t *t = a.ts[f] + g.row_off;
        uint8_t *fl = a.flags[f] + g.row_off;
        long long cnt = 0;
        for (int64_t j0 = 0; j0 < g.nrows; j0 += CM_TILE) {
            const int64_t je = j0 + CM_TILE < g.nrows ? j0 + CM_TILE
                                                      : g.nrows;
            /* this lane's elements: j0+tid, j0+tid+256, ... (sorted) */
            int64_t x[CM_TILE / 256];
            bool own[CM_TILE / 256];
            int ne = 0;
            for (int64_t j = j0 + threadIdx.x; j < je; j += blockDim.x) {
                x[ne] = t[j];
                own[ne] = true;
                if (j > 0 && t[j - 1] >= x[ne])
                    atomicOr(err, DERR_FORMAT); /* "not sorted" */
                ne++;
            }
            const int64_t x_lo = t[j0], x_hi = t[je - 1];
            for (int f2 = f + 1; f2 < nsets; f2++) {
                DevGroup g2 = a.groups[f2][s];
                const int64_t *t2 = a.ts[f2] + g2.row_off;
                const int64_t n2 = g2.nrows;
                if (n2 == 0) continue;
                int64_t wl, wend;
                cm_window(t2, n2, x_lo, x_hi, wb_sh, wl, wend);
                int k = 0; /* this lane's next unresolved element */
                for (int64_t wbase = wl; wbase < wend; wbase += CM_W) {
                    const int wcnt = int(wend - wbase < CM_W ? wend - wbase
                                                             : CM_W);
                    for (int i = threadIdx.x; i < wcnt; i += blockDim.x)
                        wts[i] = t2[wbase + i];
                    __syncthreads();
                    const int64_t w_last = wts[wcnt - 1];
                    const bool last_chunk = wbase + wcnt == wend;
                    while (k < ne && (x[k] <= w_last || last_chunk)) {
                        const int lo = cm_lower_bound(wts, wcnt, x[k]);
                        if (lo < wcnt && wts[lo] == x[k]) own[k] = false;
                        k++;
                    }
                    __syncthreads();
                }
            }
            for (int i = 0; i < ne; i++) {
                fl[j0 + threadIdx.x + int64_t(i) * blockDim.x] = own[i];
                cnt += own[i];
            }
            __syncthreads();
        }
        /* block reduce cnt -> counts[f][s] */
        sred[threadIdx.x] = cnt;
        __syncthreads();
        for (int w = blockDim.x >> 1; w > 0; w >>= 1) {
            if (threadIdx.x < unsigned(w)) sred[threadIdx.x] += sred[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0)
            a.counts[size_t(f) * nseries + s] = sred[0];
        __syncthreads();
    }
}

/* block per (set, series): exclusive block-scan of owner flags */
__global__ void k_cm_prefix(CompactArgs a, int nsets, int nseries) {
    __shared__ int32_t sh[256];
    __shared__ int32_t carry;
    int total = nsets * nseries;
    for (int idx = blockIdx.x; idx < total; idx += gridDim.x) {
        int f = idx / nseries, s = idx % nseries;
        DevGroup g = a.groups[f][s];
        const uint8_t *fl = a.flags[f] + g.row_off;
        int32_t *pf = a.prefix[f] + g.row_off;
        if (threadIdx.x == 0) carry = 0;
        __syncthreads();
        for (int64_t tile = 0; tile < g.nrows; tile += blockDim.x) {
            int64_t j = tile + threadIdx.x;
            int32_t v = (j < g.nrows) ? fl[j] : 0;
            sh[threadIdx.x] = v;
            __syncthreads();
            for (int off = 1; off < int(blockDim.x); off <<= 1) {
                int32_t u = threadIdx.x >= unsigned(off)
                                ? sh[threadIdx.x - off] : 0;
                __syncthreads();
                sh[threadIdx.x] += u;
                __syncthreads();
            }
            if (j < g.nrows)
                pf[j] = carry + sh[threadIdx.x] - v; /* exclusive */
            __syncthreads();
            if (threadIdx.x == 0) carry += sh[blockDim.x - 1];
            __syncthreads();
        }
    }
}

/* ---- scatter (gs_compact_merge_fields; gs_compact_merge is its
 * one-column case) ----
 * A column group is a time column plus every field column of the table;
 * BatchMergeBuilder::take_last_and_merge (batch_builder.rs:132-155)
 * resolves each column independently over the rows sharing a timestamp:
 * per column the newest non-null value wins.  Owner flags and prefixes
 * depend on timestamps only, so k_cm_flags/k_cm_prefix run once for any
 * ncols; only the scatter differs.
 *
 * The (stream x column) pointer table is up to 16*32*2 pointers — too big
 * for a by-value argument, so it lives in device memory:
 *   val[f*ncols+c], valid[f*ncols+c]  (NULL val = column absent in f,
 *   NULL valid = all rows valid), out_val[c], out_valid[c]. */
struct CompactFieldsArgs {
    CompactArgs m;
    const void *const *val;      /* device [nsets*ncols] */
    const uint8_t *const *valid; /* device [nsets*ncols] */
    void *const *out_val;        /* device [ncols] */
    uint8_t *const *out_valid;   /* device [ncols], entries may be NULL */
    uint32_t wide;               /* bit c set: 8-byte column, else 1-byte */
    int32_t ncols;
};

/* raw-bit move of one cell; no arithmetic touches a value */
__device__ __forceinline__ void cm_move_cell(void *dst, int64_t dpos,
                                             const void *src, int64_t srow,
                                             bool wide) {
    if (wide)
        ((uint64_t *)dst)[dpos] = ((const uint64_t *)src)[srow];
    else
        ((uint8_t *)dst)[dpos] = ((const uint8_t *)src)[srow];
}

/* Same tiling as k_cm_flags (CM_TILE stream-f elements, 8 per lane; the
 * window of every other stream staged once in LDS, with its prefix and
 * flag windows, so the rank adds are LDS reads too).  A lane cannot hold
 * ncols x 8 pending values, so values resolve against the final position:
 *   1. rank pass over all other streams -> pos; older-stream hits are
 *      kept as a 16-bit mask per element
 *   2. the owner stores out_ts and its own stream's valid columns; the
 *      rest (null or absent in f) form a 32-bit unresolved mask
 *   3. walk-back f-1 .. 0: a block vote skips streams (and, for
 *      all-valid data, the whole step) that no unresolved element hits;
 *      on a hit every unresolved column valid there is stored straight
 *      to out[c][pos] and its bit cleared
 *   4. leftovers get the zero value and validity 0.
 * Every output cell is stored exactly once, in a fixed order, with plain
 * stores.  Per-lane arrays are only ever indexed by unrolled constants
 * (a done-mask, not a running index, tracks a lane's progress), so they
 * stay in VGPRs: no scratch. */
__global__ void __launch_bounds__(256)
k_cm_scatter_fields(CompactFieldsArgs a, int nsets, int nseries,
                    int64_t *__restrict__ out_ts) {
    constexpr int NE = CM_TILE / 256;
    __shared__ int64_t wts[CM_W];
    __shared__ int32_t wpf[CM_W];
    __shared__ uint8_t wfl[CM_W];
    __shared__ int64_t wb_sh[2];
    const int f = blockIdx.y;
    const int ncols = a.ncols;
    for (int s = blockIdx.x; s < nseries; s += gridDim.x) {
        const DevGroup g = a.m.groups[f][s];
        const int64_t *t = a.m.ts[f] + g.row_off;
        const uint8_t *fl = a.m.flags[f] + g.row_off;
        const int32_t *pf = a.m.prefix[f] + g.row_off;
        const int64_t base = a.m.out_off[s];
        for (int64_t j0 = 0; j0 < g.nrows; j0 += CM_TILE) {
            const int64_t je = j0 + CM_TILE < g.nrows ? j0 + CM_TILE
                                                      : g.nrows;
            int64_t x[NE], pos[NE];
            uint32_t unres[NE];
            uint16_t hit[NE];
            uint32_t ownm = 0; /* bit i: element i exists and owns its row */
#pragma unroll
            for (int i = 0; i < NE; i++) {
                const int64_t j = j0 + threadIdx.x + int64_t(i) * 256;
                x[i] = 0;
                pos[i] = 0;
                unres[i] = 0;
                hit[i] = 0;
                if (j < je) {
                    x[i] = t[j];
                    pos[i] = base + pf[j];
                    if (fl[j]) ownm |= 1u << i;
                }
            }
            const int64_t x_lo = t[j0], x_hi = t[je - 1];

            /* 1. rank over every other stream + older-stream hit masks */
            for (int f2 = nsets - 1; f2 >= 0; f2--) {
                if (f2 == f) continue;
                const DevGroup g2 = a.m.groups[f2][s];
                const int64_t *t2 = a.m.ts[f2] + g2.row_off;
                const int32_t *pf2 = a.m.prefix[f2] + g2.row_off;
                const uint8_t *fl2 = a.m.flags[f2] + g2.row_off;
                const int64_t n2 = g2.nrows;
                if (n2 == 0) continue;
                int64_t wl, wend;
                cm_window(t2, n2, x_lo, x_hi, wb_sh, wl, wend);
                if (wl == wend) { /* tile range absent from t2: rank only */
                    if (wl > 0) {
                        const int64_t add = pf2[wl - 1] + fl2[wl - 1];
#pragma unroll
                        for (int i = 0; i < NE; i++)
                            if (ownm >> i & 1) pos[i] += add;
                    }
                    continue;
                }
                uint32_t todo = ownm; /* non-owners need no rank */
                for (int64_t wbase = wl; wbase < wend; wbase += CM_W) {
                    const int wcnt = int(wend - wbase < CM_W ? wend - wbase
                                                             : CM_W);
                    for (int i = threadIdx.x; i < wcnt; i += blockDim.x) {
                        wts[i] = t2[wbase + i];
                        wpf[i] = pf2[wbase + i];
                        wfl[i] = fl2[wbase + i];
                    }
                    __syncthreads();
                    const int64_t w_last = wts[wcnt - 1];
                    const bool last_chunk = wbase + wcnt == wend;
#pragma unroll
                    for (int i = 0; i < NE; i++) {
                        if (!(todo >> i & 1) ||
                            !(x[i] <= w_last || last_chunk))
                            continue;
                        todo &= ~(1u << i);
                        const int lo = cm_lower_bound(wts, wcnt, x[i]);
                        const int64_t p2 = wbase + lo;
                        if (lo > 0)
                            pos[i] += wpf[lo - 1] + wfl[lo - 1];
                        else if (p2 > 0)
                            pos[i] += pf2[p2 - 1] + fl2[p2 - 1];
                        if (f2 < f && lo < wcnt && wts[lo] == x[i])
                            hit[i] |= uint16_t(1u << f2);
                    }
                    __syncthreads();
                }
            }

            /* 2. own row: ts + this stream's valid columns */
#pragma unroll
            for (int i = 0; i < NE; i++)
                if (ownm >> i & 1) out_ts[pos[i]] = x[i];
            for (int c = 0; c < ncols; c++) {
                const void *src = a.val[f * ncols + c];
                const uint8_t *vd = a.valid[f * ncols + c];
                void *dst = a.out_val[c];
                uint8_t *dvd = a.out_valid[c];
                const bool wide = a.wide >> c & 1;
#pragma unroll
                for (int i = 0; i < NE; i++) {
                    if (!(ownm >> i & 1)) continue;
                    const int64_t row =
                        g.row_off + j0 + threadIdx.x + int64_t(i) * 256;
                    if (src && (!vd || vd[row])) {
                        cm_move_cell(dst, pos[i], src, row, wide);
                        if (dvd) dvd[pos[i]] = 1;
                    } else {
                        unres[i] |= 1u << c;
                    }
                }
            }

            /* 3. walk-back over older streams, newest first */
            uint32_t need = 0; /* older streams some unresolved element hits */
#pragma unroll
            for (int i = 0; i < NE; i++)
                if (unres[i]) need |= hit[i];
            if (__syncthreads_or(need != 0)) {
                for (int f2 = f - 1; f2 >= 0; f2--) {
                    need = 0;
#pragma unroll
                    for (int i = 0; i < NE; i++)
                        if (unres[i]) need |= hit[i];
                    if (!__syncthreads_or(need >> f2 & 1)) continue;
                    const DevGroup g2 = a.m.groups[f2][s];
                    const int64_t *t2 = a.m.ts[f2] + g2.row_off;
                    const int64_t n2 = g2.nrows;
                    int64_t wl, wend;
                    cm_window(t2, n2, x_lo, x_hi, wb_sh, wl, wend);
                    uint32_t todo = 0;
#pragma unroll
                    for (int i = 0; i < NE; i++)
                        if (unres[i] && (hit[i] >> f2 & 1)) todo |= 1u << i;
                    for (int64_t wbase = wl; wbase < wend; wbase += CM_W) {
                        const int wcnt = int(wend - wbase < CM_W
                                                 ? wend - wbase : CM_W);
                        for (int i = threadIdx.x; i < wcnt; i += blockDim.x)
                            wts[i] = t2[wbase + i];
                        __syncthreads();
                        const int64_t w_last = wts[wcnt - 1];
                        const bool last_chunk = wbase + wcnt == wend;
#pragma unroll
                        for (int i = 0; i < NE; i++) {
                            if (!(todo >> i & 1) ||
                                !(x[i] <= w_last || last_chunk))
                                continue;
                            todo &= ~(1u << i);
                            const int lo = cm_lower_bound(wts, wcnt, x[i]);
                            if (lo >= wcnt || wts[lo] != x[i]) continue;
                            const int64_t row2 = g2.row_off + wbase + lo;
                            for (int c = 0; c < ncols; c++) {
                                if (!(unres[i] >> c & 1)) continue;
                                const void *src = a.val[f2 * ncols + c];
                                const uint8_t *vd = a.valid[f2 * ncols + c];
                                if (!src || (vd && !vd[row2])) continue;
                                cm_move_cell(a.out_val[c], pos[i], src, row2,
                                             a.wide >> c & 1);
                                uint8_t *dvd = a.out_valid[c];
                                if (dvd) dvd[pos[i]] = 1;
                                unres[i] &= ~(1u << c);
                            }
                        }
                        __syncthreads();
                    }
                }
            }

            /* 4. leftovers: null in every stream holding the timestamp */
            for (int c = 0; c < ncols; c++) {
                void *dst = a.out_val[c];
                uint8_t *dvd = a.out_valid[c];
                const bool wide = a.wide >> c & 1;
#pragma unroll
                for (int i = 0; i < NE; i++) {
                    if (!(unres[i] >> c & 1)) continue;
                    if (wide) ((uint64_t *)dst)[pos[i]] = 0;
                    else ((uint8_t *)dst)[pos[i]] = 0;
                    if (dvd) dvd[pos[i]] = 0;
                }
            }
            __syncthreads();
        }
    }
}

/* ---- string columns in the merge (gs_compact_merge_group).  To
 * k_cm_scatter_fields a string column is an 8-byte column whose cell is a
 * reference to the winning row: 1 + (stream << 48 | row), 0 for a null
 * cell (the value the scatter's leftovers step stores).  The references of
 * stream f are the same for each of its string columns, so one array per
 * stream is materialised and the scatter kernel is the one the fixed-width
 * columns run, unchanged.  Lengths, the offsets scan and the byte gather
 * then run over the output rows only, with plain stores. */
#define CM_REF_ROW_MASK ((1ULL << 48) - 1)

struct CmStrSrc {
    const int64_t *off[GS_MAX_STREAMS];
    const uint8_t *bytes[GS_MAX_STREAMS];
};

__global__ void k_cm_str_refs(uint64_t *__restrict__ ref, int64_t rows, int f) {
    for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r < rows;
         r += int64_t(gridDim.x) * blockDim.x)
        ref[r] = ((uint64_t(f) << 48) | uint64_t(r)) + 1;
}

__global__ void k_cm_str_lens(CmStrSrc s, const uint64_t *__restrict__ ref,
                              int64_t n, int64_t *__restrict__ len) {
    for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r < n;
         r += int64_t(gridDim.x) * blockDim.x) {
        const uint64_t x = ref[r];
        int64_t l = 0;
        if (x) {
            const int64_t *o = s.off[(x - 1) >> 48] + ((x - 1) & CM_REF_ROW_MASK);
            l = o[1] - o[0];
        }
        len[r] = l;
    }
}

/* k_str_gather's copy with a per-row source base; byte by byte, since
 * neither side has any alignment */
__global__ void k_cm_str_gather(CmStrSrc s, const uint64_t *__restrict__ ref,
                                const int64_t *__restrict__ off, int64_t n,
                                uint8_t *__restrict__ out) {
    for (int64_t r = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; r < n;
         r += int64_t(gridDim.x) * blockDim.x) {
        const uint64_t x = ref[r];
        if (!x) continue;
        const int f = int((x - 1) >> 48);
        const int64_t so = s.off[f][(x - 1) & CM_REF_ROW_MASK];
        const int64_t n2 = off[r + 1] - off[r];
        const uint8_t *src = s.bytes[f] + so;
        uint8_t *d = out + off[r];
#pragma clang loop vectorize(disable) interleave(disable)
        for (int64_t k = 0; k < n2; k++) d[k] = src[k];
    }
}

/* --------------------------------------------------- fused filtered scan
 * Fast path of gs_scan when every ts page is RLE (the TSBS shape), every
 * field page is all-valid Gorilla and no tombstones apply: the span of
 * the closed time range is computed from the RLE header in closed form
 * (no ts materialization), the Gorilla decoder writes ONLY the selected
 * rows, already compacted, and the aggregate runs over the compacted
 * output — the decode work is identical (every record is still parsed;
 * only the stores of filtered-out rows are skipped), which is exactly the
 * operator fusion the north star asks for. */

/* two-level device exclusive scan of int64 counts (n <= 2048*2048);
 * out has n+1 entries, out[n] = total */
#define SCAN_BLOCK 256
#define SCAN_ITEMS 8
__global__ void k_scan_partials(const int64_t *__restrict__ in, int n,
                                int64_t *__restrict__ out,
                                int64_t *__restrict__ blocksums) {
    __shared__ int64_t sh[SCAN_BLOCK];
    int chunk = SCAN_BLOCK * SCAN_ITEMS;
    int base = blockIdx.x * chunk;
    int64_t vals[SCAN_ITEMS];
    int64_t acc = 0;
    for (int k = 0; k < SCAN_ITEMS; k++) {
        int i = base + threadIdx.x * SCAN_ITEMS + k;
        vals[k] = acc;
        acc += (i < n) ? in[i] : 0;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    /* block scan (exclusive) over per-thread sums */
    for (int off = 1; off < SCAN_BLOCK; off <<= 1) {
        int64_t v = (threadIdx.x >= unsigned(off)) ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += v;
        __syncthreads();
    }
    int64_t tbase = (threadIdx.x > 0) ? sh[threadIdx.x - 1] : 0;
    for (int k = 0; k < SCAN_ITEMS; k++) {
        int i = base + threadIdx.x * SCAN_ITEMS + k;
        if (i < n) out[i] = tbase + vals[k];
    }
    if (threadIdx.x == SCAN_BLOCK - 1) blocksums[blockIdx.x] = sh[threadIdx.x];
}

__global__ void k_scan_fixup(int n, int64_t *__restrict__ out,
                             int64_t *__restrict__ blocksums, int nblocks) {
    /* one wave: shuffle-scan the block sums in 64-wide tiles with a
       running carry (exact integer prefix — order fixed).  Handles the
       large-row string decode scans (tens of thousands of blocks)
       without a serial single-thread walk. */
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    int64_t carry = 0;
    for (int t = 0; t < nblocks; t += 64) {
        int i = t + lane;
        int64_t v = (i < nblocks) ? blocksums[i] : 0;
        int64_t x = v;
        for (int off = 1; off < 64; off <<= 1) {
            int64_t u = __shfl_up(x, off, 64);
            if (lane >= off) x += u;
        }
        if (i < nblocks) blocksums[i] = carry + x - v; /* exclusive */
        carry += __shfl(x, 63, 64);
    }
    if (lane == 0) out[n] = carry; /* total */
}

__global__ void k_scan_add(int n, int64_t *__restrict__ out,
                           const int64_t *__restrict__ blocksums) {
    int chunk = SCAN_BLOCK * SCAN_ITEMS;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += gridDim.x * blockDim.x)
        out[i] += blocksums[i / chunk];
}

/* series-group layout of the fused compacted output, built on device:
 * sgroup s covers page-groups [first[s], first[s+1]) */
__global__ void k_build_sgroups_out(const int32_t *__restrict__ first,
                                    int nsg,
                                    const int64_t *__restrict__ out_off,
                                    DevGroup *__restrict__ sg) {
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < nsg;
         s += gridDim.x * blockDim.x) {
        int64_t a = out_off[first[s]];
        int64_t b = out_off[first[s + 1]];
        sg[s].row_off = a;
        sg[s].nrows = int32_t(b - a);
        sg[s].pad = 0;
    }
}

/* closed-form span of closed [lo,hi] on an RLE ts page */
__global__ void k_spans_rle(const uint8_t *__restrict__ blob,
                            const DevPage *__restrict__ pages, int npages,
                            int64_t lo, int64_t hi,
                            int64_t *__restrict__ sp_start,
                            int64_t *__restrict__ sp_cnt,
                            int64_t *__restrict__ g_t0sel,
                            int64_t *__restrict__ g_delta,
                            unsigned *__restrict__ err) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npages;
         p += gridDim.x * blockDim.x) {
        DevPage pg = pages[p];
        /* a page gs_decode refuses is refused here alike: empty span, and
           the scan fails at its check of err */
        const IntHeader h =
            int_page_header(blob + pg.data_off, pg.data_len, pg.enc);
        const int64_t first = h.first, delta = h.rle_delta;
        int64_t n = pg.nrows;
        int64_t st, en; /* selected rows = [st, en) */
        if (h.verdict) { atomicOr(err, h.verdict); st = en = 0; }
        else if (delta < 0) { atomicOr(err, DERR_NONMONO); st = en = 0; }
        else if (delta == 0) {
            bool in = first >= lo && first <= hi;
            st = 0; en = in ? n : 0;
        } else {
            __int128 d = delta;
            __int128 a = (__int128)lo - first;
            __int128 b = (__int128)hi - first;
            __int128 s0 = a <= 0 ? 0 : (a + d - 1) / d; /* ceil */
            __int128 e0 = b < 0 ? 0 : b / d + 1;        /* floor + 1 */
            if (s0 > n) s0 = n;
            if (e0 > n) e0 = n;
            st = int64_t(s0);
            en = int64_t(e0);
        }
        if (en < st) en = st;
        sp_start[pg.grp] = st;
        sp_cnt[pg.grp] = en - st;
        /* RLE grid of the SELECTED rows, for the closed-form aggregate
           boundary computation (k_agg_partial_rle) */
        g_t0sel[pg.grp] = first + st * delta;
        g_delta[pg.grp] = delta;
    }
}

#define GS_TS_TILE 16384 /* output rows per work item of k_rle_ts_tiles */

/* First non-empty page-group at or after g0 whose compacted rows reach past
 * output row r: the smallest g in [g0, ngroups) with out_off[g + 1] > r.
 * The caller guarantees r < out_off[ngroups].  Uniform over the block (the
 * loads are scalar); out_off is small enough to stay in L2. */
__device__ __forceinline__ int ts_group_of(const int64_t *__restrict__ out_off,
                                           int g0, int ngroups, int64_t r) {
    int lo = g0, hi = ngroups - 1;
    while (lo < hi) {
        int mid = lo + ((hi - lo) >> 1);
        if (out_off[mid + 1] > r) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

/* RLE ts generation of only the selected spans, compacted.  The work item
 * is a tile of `tile` OUTPUT rows, not a page: every block stores the same
 * number of bytes whatever the page size, the pages per series or the
 * selection (one block per page left half the chip idle whenever the page
 * index modulo the grid lined up with the selected pages).  Row j of group
 * g is g_t0sel[g] + j * g_delta[g] (k_spans_rle), so no page header is
 * read here.  A tile finds its first group by binary search in out_off and
 * walks forward; runs of empty groups are skipped by another search.
 * Writes exactly rows [out_off[0], out_off[ngroups]). */
__global__ __launch_bounds__(256) void k_rle_ts_tiles(
    const int64_t *__restrict__ out_off, int ngroups,
    const int64_t *__restrict__ g_t0sel, const int64_t *__restrict__ g_delta,
    int tile, int64_t *__restrict__ out_ts) {
    const int64_t first = out_off[0];
    const int64_t total = out_off[ngroups];
    const int64_t ntiles = (total - first + tile - 1) / tile;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        int64_t r = first + t * tile;
        const int64_t r_end = r + tile < total ? r + tile : total;
        int g = ts_group_of(out_off, 0, ngroups, r);
        while (true) {
            /* rows [r, seg_end) of group g, which holds row r */
            const int64_t g_first = out_off[g], g_end = out_off[g + 1];
            const int64_t seg_end = g_end < r_end ? g_end : r_end;
            const int64_t cnt = seg_end - r;
            const uint64_t delta = uint64_t(g_delta[g]);
            const uint64_t base =
                uint64_t(g_t0sel[g]) + uint64_t(r - g_first) * delta;
            int64_t *o = out_ts + r;
            /* paired 16-B stores: closed-form generation is pure store
               bandwidth; halving the store-instruction count lifted the
               measured rate (the 1-row peel goes by the destination
               address, so a caller's 8-B-aligned buffer is as good as a
               16-B one).  One multiply per lane and segment; the loop
               itself only adds. */
            const int64_t head = int64_t((uintptr_t(o) >> 3) & 1);
            if (head && threadIdx.x == 0) o[0] = int64_t(base);
            const int64_t n2 = (cnt - head) >> 1;
            longlong2 *op = (longlong2 *)(o + head);
            uint64_t v0 =
                base + (uint64_t(head) + 2 * uint64_t(threadIdx.x)) * delta;
            const uint64_t step = 2 * uint64_t(blockDim.x) * delta;
            for (int64_t q2 = threadIdx.x; q2 < n2; q2 += blockDim.x) {
                longlong2 v;
                v.x = int64_t(v0);
                v.y = int64_t(v0 + delta);
                op[q2] = v;
                v0 += step;
            }
            if (((cnt - head) & 1) && threadIdx.x == 0)
                o[cnt - 1] = int64_t(base + uint64_t(cnt - 1) * delta);
            r = seg_end;
            if (r >= r_end) break;
            /* the next group is usually not empty: look before searching */
            g = out_off[g + 2] > r ? g + 1
                                   : ts_group_of(out_off, g + 2, ngroups, r);
        }
    }
}

/* Sub-page pruning for the fused scan: compact the indices of chunks whose
 * row range overlaps their group's selected span (the chunk-granularity
 * analog of the reference's page min/max pruning, reader/chunk.rs:12-49 —
 * a chunk wholly outside the time range is never parsed at all).  Output
 * order is wave-compacted (near table order); chunks write disjoint
 * output rows so order never affects results.  With the fused aggregate
 * (pieces != nullptr) a chunk left out of the list gets its two piece
 * slots marked absent here, so nothing survives from an earlier scan with
 * another time range. */
__global__ void k_gor_active(const DevGorChunk *__restrict__ chunks,
                             int nchunks,
                             const int64_t *__restrict__ sp_start,
                             const int64_t *__restrict__ sp_cnt,
                             int *__restrict__ active,
                             int *__restrict__ n_active,
                             DevAggMeta *__restrict__ pieces) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nchunks;
         i += gridDim.x * blockDim.x) {
        uint32_t grp = chunks[i].grp;
        int64_t row0 = int64_t(chunks[i].row0);
        int64_t rend = row0 + int64_t(chunks[i].cnt);
        int64_t lo = sp_start[grp];
        int64_t hi = lo + sp_cnt[grp];
        bool act = row0 < hi && rend > lo;
        if (pieces && !act) {
            uint32_t slot = chunks[i].slot;
            if (slot != GOR_NO_SLOT) /* both pieces: one 16-B store */
                *(int4 *)(pieces + 2 * size_t(slot)) =
                    make_int4(AGG_NO_PIECE, 0, AGG_NO_PIECE, 0);
        }
        uint64_t m = __ballot(act);
        if (m) {
            int leader = __ffsll((unsigned long long)m) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(n_active, __popcll(m));
            base = __shfl(base, leader);
            if (act)
                active[base + __popcll(m & ((1ull << lane) - 1))] = i;
        }
    }
}

/* Chunk-parallel Gorilla decode writing only the selected span, compacted
 * (same LDS flush as k_gor_chunks; each lane's staged run is contiguous
 * in the output by construction).  Runs over the k_gor_active index list;
 * rows before the span are parsed but not staged (the bitstream is
 * sequential), and a chunk whose decodability was proven by the upload
 * pre-pass (safe_stop) stops as soon as the span's end is passed.
 *
 * AGG = true also aggregates the staged rows into the scan's time buckets
 * while they sit in the lane's registers, so no later kernel has to read
 * the 8 B/row it just wrote.  A page's ts is first + r*delta, so the row
 * at which bucket k starts is ceil((t0 + k*bucket_ns - first) / delta):
 * two wide divisions per chunk at init, then each further boundary by
 * adding bucket_ns/delta and carrying the remainder (no division in the
 * row loop).  A lane keeps a running max/sum of the current piece; at a
 * boundary the finished piece goes to the chunk's head slot if it is the
 * chunk's first, else straight into its (sgroup, bucket) cell — a bucket
 * strictly inside one chunk's rows is complete for the series.  The last
 * piece goes to the tail slot (DevAggMeta/DevAggVal; k_agg_fixup).  Rows before t0
 * accumulate into pseudo bucket -1 and rows past the grid into bucket
 * n_buckets; neither is ever stored as a cell. */
struct GorAggArgs {
    const int32_t *grp_sg;  /* page-group -> series group */
    const int64_t *g_t0sel; /* k_spans_rle: ts of first selected row */
    const int64_t *g_delta; /* k_spans_rle: RLE delta */
    int64_t t0, bucket_ns;
    int nbuckets;
    double *pmax, *psum;
    long long *pcnt;
    DevAggMeta *pc_meta; /* [2*slot], [2*slot+1]: head, tail */
    DevAggVal *pc_val;
};

/* Fewest rows a bucket must span (bucket_ns / smallest positive RLE delta
 * of the set) for the fused aggregate to be chosen; below it the scan
 * launches k_agg_partial_rle as before.  Measured on MI355X, 16384 series
 * x 3 pages x 4500 rows, middle half selected, decode+aggregate ms of one
 * scan (fused / separate): 300 rows per bucket 2.94 / 2.98, 64: 2.99 /
 * 3.40, 16: 3.35 / 5.16, 8: 4.07 / 7.61, 4: 5.83 / 12.6, 2: 9.28 / 22.9.
 * A boundary costs no division here, and the separate pass pays a 64-lane
 * shuffle tree per bucket, so no crossover was found: the fused path led
 * at every size measured.  Below 2 rows per bucket nothing was measured
 * (n_buckets > 8192 at that shape), so that range keeps the old path. */
#define GS_AGG_FUSED_MIN_ROWS 2

/* k_gor_chunks_filtered: window bit count of a parked lane (never drops
 * below 64, so a parked lane never refills), and what a lane's stop row S
 * stands for */
#define GOR_PARK_NB (1 << 30)
#define GOR_FK_END 0   /* the chunk's own end: check the bit count */
#define GOR_FK_CLEAN 1 /* span end inside a GORF_SAFE_STOP chunk: no check */
#define GOR_FK_OVER 2  /* the refill overran the stream: always an error */

template <bool AGG>
__global__ void k_gor_chunks_filtered(const uint8_t *__restrict__ blob,
                                      const DevGorChunk *__restrict__ chunks,
                                      const int *__restrict__ active,
                                      const int *__restrict__ n_active,
                                      const int64_t *__restrict__ sp_start,
                                      const int64_t *__restrict__ sp_cnt,
                                      const int64_t *__restrict__ out_off,
                                      double *__restrict__ out,
                                      unsigned *__restrict__ err,
                                      GorAggArgs ag) {
    __shared__ double ring[GS_GOR_BLOCK / 64][GS_RING][64 + 1];
    /* per-flush lane descriptors: {element offset into out, staged count}
       packed so the flush loop reads ONE broadcast ds_read per source lane
       instead of three cross-lane shuffles.  An offset, not a pointer: a
       pointer that travels through LDS loses its address space and the
       stores become flat (counted against lgkmcnt as well as vmcnt). */
    __shared__ uint64_t fdesc[GS_GOR_BLOCK / 64][64][2];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    auto rslot = ring[wv];
    const int nact = *n_active;
    int stride = gridDim.x * blockDim.x;
    int base_id = blockIdx.x * blockDim.x + threadIdx.x;
    int rounds = (nact + stride - 1) / stride;
    for (int rd = 0; rd < rounds; rd++) {
        int ai = base_id + rd * stride;
        bool have = ai < nact;
        /* branch-free prologue: clamp to entry 0 so every load issues
           unconditionally and the compiler batches them under one wait
           (the predicated version serialized ~5 dependent vmcnt(0)s) */
        DevGorChunk ch = chunks[active[have ? ai : 0]];
        /* spans/rows are page-local (< 2^31): 32-bit compares in the
           per-value hot loop */
        int32_t sel_lo = int32_t(sp_start[ch.grp]);
        int32_t sel_hi = int32_t(sel_lo + sp_cnt[ch.grp]);
        if (!have) { sel_lo = 0; sel_hi = 0; }
        int32_t r = int32_t(ch.row0);
        const int32_t end = r + int32_t(ch.cnt);
        /* rows [sel_lo, stage_hi) of this chunk are staged; the staged run
           is contiguous, so the output cursor only ever advances by the
           count of each flush */
        const int32_t stage_hi = sel_hi < end ? sel_hi : end;
        const uint32_t span_w =
            stage_hi > sel_lo ? uint32_t(stage_hi - sel_lo) : 0u;
        uint64_t o_cur = uint64_t(out_off[ch.grp]) +
                         uint64_t((r > sel_lo ? r : sel_lo) - sel_lo);
        GorChunkState st;
        gor_position(st, blob, ch);
        bool live = have && ch.cnt > 0;
        if (live && st.bad) { atomicOr(err, DERR_SHORT); live = false; }
        /* Refill state.  The 128-bit window hi:lo holds nb valid bits;
           nextw is the next big-endian word, raw2 the one after it exactly
           as loaded (swapped only when it is promoted to nextw, so nothing
           touches the loaded register before the following refill and the
           load latency hides behind a whole refill interval).  pl is the
           address of the next load and stops at the last loadable word;
           wrem counts the words left before the zero clamp, standing in
           for GorChunkState's p: wrem > 0 <=> p < p_clamp, and
           wrem <= -3 <=> a refill has found p >= p_over. */
        uint64_t hi = 0, lo = 0, nextw = 0, raw2 = 0, val = 0;
        int nb = GOR_PARK_NB;
        uint32_t trailing = 0, meaningful = 64;
        const uint8_t *pl = blob;
        int32_t wrem = 0;
        /* One stop row per chunk instead of per-row end tests: a chunk
           that is not its page's last stops at its own end (fk END, the
           bit count is checked there), a chunk the pre-pass proved
           decodable at the span end if that comes first (fk CLEAN, no
           check).  A last chunk without either parses on to the sentinel. */
        int32_t S = INT32_MAX;
        int fk = GOR_FK_END;
        if (live) {
            hi = st.hi; lo = st.lo; nb = st.nb;
            nextw = st.nextw;
            raw2 = __builtin_bswap64(st.nextw2);
            val = st.val;
            trailing = st.trailing;
            meaningful = st.meaningful;
            wrem = int32_t((st.p_clamp - st.p) >> 3);
            pl = st.p;
            if (ch.row0 == 0) {
                /* the page's first value comes from the header: one zero
                   control bit in front of the stream makes the first
                   iteration parse it as a repeat of val, so the header
                   row takes the same path as every other row (once it is
                   consumed the bit accounting is that of the real stream) */
                nb = 1;
            }
            if (!ch.last) S = end;
            if ((ch.flags & GORF_SAFE_STOP) && sel_hi < S) {
                S = sel_hi;
                fk = GOR_FK_CLEAN;
            }
        } else {
            r = INT32_MIN; /* parked from the start */
        }
        /* AGG: current piece = rows [a_start, r) of bucket a_b; a_next is
           the page-local row at which bucket a_b+1 starts, a_slack how far
           (ns) that row lies past the boundary itself.  a_next is held at
           INT32_MAX once it reaches stage_hi: a boundary row that is never
           staged never closes a piece. */
        int32_t a_b = -1, a_next = INT32_MAX, a_start = 0;
        double a_mx = -__builtin_inf(), a_sm = 0.0;
        uint64_t a_slack = 0, a_rem = 0, a_d = 0;
        uint32_t a_q = 0;
        size_t a_cell0 = 0;
        bool a_head = false; /* the chunk's head slot has been written */
        if (AGG && have) {
            const int64_t d = ag.g_delta[ch.grp];
            const int32_t r0 = int32_t(ch.row0);
            const int32_t rs = r0 > sel_lo ? r0 : sel_lo; /* first staged row */
            a_start = rs;
            a_cell0 = size_t(ag.grp_sg[ch.grp]) * size_t(ag.nbuckets);
            /* ts of row rs relative to the grid origin */
            const __int128 x = (__int128)ag.g_t0sel[ch.grp] +
                               (__int128)(rs - sel_lo) * d - ag.t0;
            __int128 kb = x < 0 ? -1 : x / ag.bucket_ns;
            if (kb > ag.nbuckets) kb = ag.nbuckets;
            a_b = int32_t(kb);
            if (d > 0 && a_b < ag.nbuckets) {
                /* ns from row rs to the start of bucket a_b+1: > 0 */
                const __int128 bound = (__int128)(a_b + 1) * ag.bucket_ns - x;
                const __int128 k = (bound + d - 1) / d; /* rows, >= 1 */
                a_slack = uint64_t(k * d - bound);
                a_next = rs + k >= stage_hi ? INT32_MAX : int32_t(rs + k);
                const uint64_t q = uint64_t(ag.bucket_ns) / uint64_t(d);
                a_q = q > INT32_MAX ? uint32_t(INT32_MAX) : uint32_t(q);
                a_rem = uint64_t(ag.bucket_ns) % uint64_t(d);
                a_d = uint64_t(d);
            }
        }
        auto agg_put = [&](size_t pi, int32_t cnt) {
            DevAggVal v;
            v.mx = a_mx;
            v.sm = a_sm;
            ag.pc_val[pi] = v;
            DevAggMeta m;
            m.bucket = a_b;
            m.cnt = cnt;
            ag.pc_meta[pi] = m;
        };
        /* row r (< stage_hi, so it will be staged) opens the next bucket:
           the piece that ends here is not the chunk's last, so it is the
           head or complete.  Loops only when a bucket is shorter than the
           row spacing (empty complete cells). */
        auto agg_boundary = [&]() {
            do {
                const int32_t cnt = r - a_start;
                if (!a_head) {
                    agg_put(2 * size_t(ch.slot), cnt);
                    a_head = true;
                } else if (a_b >= 0) { /* a_b < nbuckets: else a_next is
                                          INT32_MAX and never reached */
                    const size_t cell = a_cell0 + size_t(a_b);
                    ag.pmax[cell] = a_mx;
                    ag.psum[cell] = a_sm;
                    ag.pcnt[cell] = cnt;
                }
                a_b++;
                a_start = r;
                a_mx = -__builtin_inf();
                a_sm = 0.0;
                if (a_b >= ag.nbuckets) {
                    a_next = INT32_MAX;
                } else {
                    int64_t nn = int64_t(a_next) + int64_t(a_q);
                    if (a_slack < a_rem) { a_slack += a_d; nn++; }
                    a_slack -= a_rem;
                    a_next = nn >= stage_hi ? INT32_MAX : int32_t(nn);
                }
            } while (a_next == r);
        };
        /* the chunk's open piece at its stop row rr is its last: its only
           one (head, no tail) or its tail.  Every active chunk writes both
           slots. */
        auto agg_tail = [&](int32_t rr) {
            const int32_t e = rr < stage_hi ? rr : stage_hi;
            const int32_t cnt = e > a_start ? e - a_start : 0;
            const size_t pi = 2 * size_t(ch.slot);
            if (!a_head) {
                agg_put(pi, cnt);
                DevAggMeta none;
                none.bucket = AGG_NO_PIECE;
                none.cnt = 0;
                ag.pc_meta[pi + 1] = none;
            } else {
                agg_put(pi + 1, cnt);
            }
        };
        if (AGG && have && !live) agg_tail(int32_t(ch.row0));
        auto topup = [&]() { /* only with nb < 64 */
            const uint64_t x = nextw;
            nextw = wrem >= 0 ? __builtin_bswap64(raw2) : 0;
            __builtin_memcpy(&raw2, pl, 8);
            pl += wrem > 1 ? 8 : 0;
            wrem--;
            /* the bits of hi below nb are zero, so nb == 0 needs no case
               of its own; (x << 1) << (63 - nb) is x << (64 - nb) without
               the undefined shift by 64 */
            hi |= x >> nb;
            lo = (x << 1) << (63 - nb);
            nb += 64;
        };
        auto consume = [&](unsigned k) { /* k in 1..=64 */
            hi = (k == 64) ? lo : ((hi << k) | (lo >> (64 - k)));
            lo = (k == 64) ? 0 : (lo << k);
            nb -= int(k);
        };
        auto fd = fdesc[wv];
        /* 4 source lanes per store instruction: lane = (sq:2, idx:4), sq
           picks the source sub-lane, idx the ring slot — the ring is 16
           deep, so a one-source-per-instruction flush leaves 48/64 lanes
           idle; this shape keeps every lane useful and issues 16 stores
           per flush instead of 64 (reads batched 4 deep before their
           stores, the earlier register-batching lesson) */
        const int f_idx = lane & (GS_RING - 1);
        const int f_sq = lane / GS_RING;
        double *const rbase = &rslot[0][lane];
        double *rcur = rbase; /* strength-reduced ring cursor */
        auto flush = [&]() {
            const int rfill = int(rcur - rbase) / 65;
            fd[lane][0] = o_cur;
            fd[lane][1] = uint64_t(rfill);
            o_cur += uint64_t(rfill);
            rcur = rbase;
            __builtin_amdgcn_wave_barrier();
            constexpr int SRCP = 64 / GS_RING; /* sources per store */
            for (int src0 = 0; src0 < 64; src0 += SRCP * 4) {
                double vbuf[4];
                uint64_t ob[4];
                int cnt[4];
                for (int t = 0; t < 4; t++) {
                    int src = src0 + f_sq + t * SRCP;
                    vbuf[t] = rslot[f_idx][src];
                    ob[t] = fd[src][0];
                    cnt[t] = int(fd[src][1]);
                }
                for (int t = 0; t < 4; t++)
                    if (f_idx < cnt[t]) out[ob[t] + uint64_t(f_idx)] = vbuf[t];
            }
            __builtin_amdgcn_wave_barrier();
        };
        /* The lane's parse is over (sent: on the sentinel, whose iteration
           staged nothing but did count a row; else at the stop row S).
           Settle the error status and the last aggregate piece here, once,
           then park: on an all-zero window every further iteration parses
           a repeat, never refills, and r < 0 lies outside every span, so a
           parked lane needs no guard in the loop. */
        auto finish = [&](bool sent) {
            const int32_t rr = sent ? r - 1 : r;
            /* bits consumed so far: words fetched minus the two staged
               ahead, minus what the window still holds */
            const int64_t total = (int64_t(ch.data_len) - 10) * 8;
            const int64_t W3 = int64_t((uint64_t(total) + 63) >> 6) + 3;
            const int64_t used = (W3 - wrem) * 64 - 128 - nb;
            bool bad;
            if (fk == GOR_FK_OVER) bad = true;
            else if (sent) bad = used > total || rr < end;
            else bad = fk == GOR_FK_END && used > total;
            if (bad) atomicOr(err, DERR_SHORT);
            if (AGG) agg_tail(rr);
            r = INT32_MIN;
            hi = 0;
            lo = 0;
            nb = GOR_PARK_NB;
            S = INT32_MAX;
            a_next = INT32_MAX;
        };
        int32_t r_evt = S < a_next ? S : a_next; /* next row with an event */
        /* GS_RING iterations stage at most GS_RING rows per lane, so one
           flush per block can never overflow the ring — no ballot, and
           the all-parked test runs once per block, not once per value */
        bool more = !__all(r < 0);
        while (more) {
            /* not unrolled: bodies unrolled 2, 4 and 16 times measured the
               same step time, so the smallest code is kept */
#pragma unroll 1
            for (int it = 0; it < GS_RING; it++) {
                if (nb < 64) topup();
                uint32_t top13 = uint32_t(hi >> 51);
                {
                    /* uniform path (no repeat/xor branch): a repeat is an
                       XOR value with 0 meaningful bits (sb=0), so every
                       lane runs the same straight-line code and the wave
                       diverges only on the rare need>64 case — measured
                       the round-1 two-branch parse at ~20% VALU
                       utilization, divergence being the dominant loss */
                    unsigned bit0 = (top13 >> 12) & 1; /* 1 = XOR value */
                    unsigned bit1 = (top13 >> 11) & 1; /* 1 = new window */
                    unsigned nw = bit0 & bit1;
                    uint32_t lead = (top13 >> 6) & 0x1f;
                    uint32_t mg_raw = top13 & 0x3f;
                    uint32_t mg_new = mg_raw ? mg_raw : 64;
                    uint32_t tr_new = mg_raw ? (64 - lead - mg_raw) : 0;
                    meaningful = nw ? mg_new : meaningful;
                    trailing = nw ? tr_new : trailing;
                    unsigned shift = bit0 ? (bit1 ? 13u : 2u) : 1u;
                    unsigned m_eff = bit0 ? meaningful : 0u;
                    unsigned need = shift + m_eff;
                    uint64_t sb;
                    if (__builtin_expect(need < 64, 1)) {
                        /* nb >= 64 after the loop-top topup; need < 64
                           keeps the consume branch-free (no k==64 case) */
                        uint64_t w = (hi << shift) | (lo >> (64 - shift));
                        /* m_eff != 0 <=> bit0: a mask, not a branch */
                        sb = (w >> ((64 - m_eff) & 63)) &
                             (uint64_t(0) - uint64_t(bit0));
                        hi = (hi << need) | (lo >> (64 - need));
                        lo <<= need;
                        nb -= int(need);
                    } else { /* m_eff >= 51: rare */
                        consume(shift);
                        while (nb < int(m_eff)) topup();
                        sb = (m_eff == 64) ? hi : (hi >> (64 - m_eff));
                        consume(m_eff);
                    }
                    val ^= sb << trailing;
                    const bool sent = bit0 && val == GORILLA_SENTINEL;
                    /* one exec region: both tests evaluated, no && */
                    if (int(!sent) &
                        int(uint32_t(r) - uint32_t(sel_lo) < span_w)) {
                        const double x = __longlong_as_double((long long)val);
                        if (AGG) {
                            if (x > a_mx) a_mx = x;
                            a_sm += x;
                        }
                        *rcur = x;
                        rcur += 65;
                    }
                    r++;
                    /* rare: the stop row, the sentinel, or (AGG) the row
                       that opens the next bucket — closed before that row
                       is staged, which is the next thing to happen */
                    if (__builtin_expect(sent || r == r_evt, 0)) {
                        if (sent || r == S) finish(sent);
                        else if (AGG) agg_boundary();
                        r_evt = S < a_next ? S : a_next;
                    }
                }
            }
            flush();
            /* overrun (a refill met p_over): reads past the clamp gave
               zeros, i.e. repeats, so nothing was harmed in between; make
               the next row this lane's stop.  Whatever else ends such a
               lane first finds used > total and reports the same error. */
            if (r >= 0 && wrem <= -3) {
                fk = GOR_FK_OVER;
                S = r + 1;
                r_evt = S;
            }
            more = !__all(r < 0);
        }
    }
}

/* Fused aggregate, second half: one block per series group walks the
 * group's chunk pieces in slot order (page-group order, then row order =
 * time order, as k_agg_partial_rle assumes too) and folds head and tail
 * pieces that share a bucket, always in that order, so the sum has one
 * fixed association however the decode lanes were scheduled.  Each such
 * cell is written once, by the thread that owns the first piece of its
 * run.  Cells the decode kernel completed itself — the buckets strictly
 * between a chunk's head and tail — are only marked; every cell left
 * unmarked received no rows and gets (-inf, 0.0, 0).  After this kernel
 * every (sgroup, bucket) cell holds this scan's value, by plain stores. */
__global__ void k_agg_fixup(const DevAggMeta *__restrict__ pc_meta,
                            const DevAggVal *__restrict__ pc_val,
                            const int32_t *__restrict__ sg_chunk_first,
                            int nsg, int nbuckets, int max_pieces,
                            double *__restrict__ pmax,
                            double *__restrict__ psum,
                            long long *__restrict__ pcnt) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int32_t *pb = (int32_t *)smem;            /* [max_pieces] bucket or -1 */
    uint8_t *done = smem + size_t(max_pieces) * 4; /* [nbuckets] */
    for (int g = blockIdx.x; g < nsg; g += gridDim.x) {
        const int c0 = sg_chunk_first[g];
        const int nch = sg_chunk_first[g + 1] - c0;
        const int np = 2 * nch;
        const DevAggMeta *gm = pc_meta + 2 * size_t(c0);
        const DevAggVal *gv = pc_val + 2 * size_t(c0);
        const size_t cell0 = size_t(g) * size_t(nbuckets);
        for (int b = threadIdx.x; b < nbuckets; b += blockDim.x) done[b] = 0;
        __syncthreads();
        for (int c = threadIdx.x; c < nch; c += blockDim.x) {
            const int4 ht = *(const int4 *)(gm + 2 * c);
            const int32_t hb = ht.x, hc = ht.y, tb = ht.z, tc = ht.w;
            const bool hok = hb >= 0 && hb < nbuckets && hc > 0;
            const bool tok = tb >= 0 && tb < nbuckets && tc > 0;
            pb[2 * c] = hok ? hb : -1;
            pb[2 * c + 1] = tok ? tb : -1;
            if (hb != AGG_NO_PIECE && tb != AGG_NO_PIECE) {
                const int lo = hb + 1 > 0 ? hb + 1 : 0;
                const int hi = tb < nbuckets ? tb : nbuckets;
                for (int b = lo; b < hi; b++) done[b] = 1;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < np; i += blockDim.x) {
            const int32_t b = pb[i];
            if (b < 0) continue;
            int j = i - 1;
            while (j >= 0 && pb[j] < 0) j--;
            if (j >= 0 && pb[j] == b) continue; /* continues an earlier run */
            double mx = gv[i].mx, sm = gv[i].sm;
            long long c = gm[i].cnt;
            for (int k = i + 1; k < np; k++) {
                const int32_t bk = pb[k];
                if (bk < 0) continue;
                if (bk != b) break;
                const double omx = gv[k].mx;
                if (omx > mx) mx = omx;
                sm += gv[k].sm;
                c += gm[k].cnt;
            }
            pmax[cell0 + b] = mx;
            psum[cell0 + b] = sm;
            pcnt[cell0 + b] = c;
            done[b] = 1;
        }
        __syncthreads();
        for (int b = threadIdx.x; b < nbuckets; b += blockDim.x)
            if (!done[b]) {
                pmax[cell0 + b] = -__builtin_inf();
                psum[cell0 + b] = 0.0;
                pcnt[cell0 + b] = 0;
            }
        __syncthreads();
    }
}

/* --------------------------------------------------- GPU page re-encode
 * The write side of compaction (tsm/writer.rs:249-314 via
 * Page::arrow_array_to_page, tsm/page.rs:100-353): one thread per output
 * page running the encoders of gs_tsm_enc.h, the functions the host entry
 * points of gs_encode.cpp run (pinned by the reference's golden vectors).
 * The encoders want all-valid input (time columns are never null;
 * k_enc_prepare densifies every null-carrying column first). */

struct EncPageSpec {
    int64_t row_off;
    int32_t nrows;
    int32_t pad;
};

/* the block's CRC table in LDS, built cooperatively */
__device__ __forceinline__ void enc_crc_table(uint32_t *crct) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        crct[i] = tsm_crc32_entry(uint32_t(i));
    __syncthreads();
}

/* Ends one page's encode.  dl is what the encoder returned: an error is
 * raised and handed on as the page's length, else the page gets its crc
 * and header (bl = bitset bytes) and its full length comes back. */
__device__ __forceinline__ int64_t enc_seal_page(
    uint8_t *pg, uint32_t bl, int32_t nrows, const uint8_t *data, int64_t dl,
    const uint32_t *crct, unsigned *err) {
    if (dl < 0) {
        atomicOr(err, dl == TSM_ENC_ERR_SENTINEL ? DERR_ENC_SENTINEL
                                                 : DERR_FORMAT);
        return dl;
    }
    tsm_page_header(pg, bl, uint64_t(nrows), tsm_crc32(crct, data, size_t(dl)));
    return 16 + int64_t(bl) + dl;
}

/* ---- column-group re-encode (gs_encode_group_pages_dev, and
 * gs_encode_pages_dev as its one-column case): every page of every column
 * of a merged column group in two launches.  k_enc_prepare
 * does the per-page work that parallelises (bitset, null densification,
 * count, statistics, bool packing), one block per (column, page);
 * k_enc_group_pages then runs the serial int/Gorilla encoders over
 * the dense values, one thread per (column, page), and seals the page. */

struct EncGroupCol {
    const void *vals;     /* 8 B/row; bool 1 B/row */
    const uint8_t *valid; /* 1 B/row, NULL = all valid */
    void *dense;          /* non-null values in row order at the page's
                             row_off; NULL when valid is NULL (the source
                             column is already dense) */
    uint8_t *out;
    int64_t cap;
    int32_t ctype;
    uint32_t flags;
};
#define ENC_COL_NO_NULLS 1u /* a null row fails the page, as in a time column */

#define ENC_PREP_THREADS 256
#define ENC_PREP_WAVES (ENC_PREP_THREADS / 64)

/* a < b / a == b in the column's own type, on raw bits */
__device__ __forceinline__ bool enc_lt(int ct, uint64_t a, uint64_t b) {
    if (ct == GS_CT_F64)
        return __longlong_as_double((long long)a) <
               __longlong_as_double((long long)b);
    if (ct == GS_CT_U64) return a < b;
    return int64_t(a) < int64_t(b);
}
__device__ __forceinline__ bool enc_eq(int ct, uint64_t a, uint64_t b) {
    if (ct == GS_CT_F64)
        return __longlong_as_double((long long)a) ==
               __longlong_as_double((long long)b);
    return a == b;
}
/* Page statistics restate a sequential loop with strict compares
 * (tsm/page.rs:137-290): of values that compare equal the FIRST in row
 * order stays (this decides the sign of a zero extremum), and a NaN never
 * compares, so it changes nothing.  (value, row) under "smaller value, then
 * smaller row" is a total order over the non-NaN values, so the reduction
 * below gives that loop's bits for any partition of the rows. */
__device__ __forceinline__ void enc_min_merge(int ct, uint64_t &a, int32_t &ra,
                                              uint64_t b, int32_t rb) {
    if (enc_lt(ct, b, a) || (enc_eq(ct, b, a) && rb < ra)) { a = b; ra = rb; }
}
__device__ __forceinline__ void enc_max_merge(int ct, uint64_t &a, int32_t &ra,
                                              uint64_t b, int32_t rb) {
    if (enc_lt(ct, a, b) || (enc_eq(ct, b, a) && rb < ra)) { a = b; ra = rb; }
}

/* One block per (column, page), work item w = c*npages + p.  Each step
 * takes ENC_PREP_THREADS rows: a wave's __ballot of the validity bytes is
 * 8 bytes of the LSB-first bitset, written straight into the page by
 * lanes 0..7; a valid row's slot in the dense column is the count of valid
 * rows before it (earlier steps + earlier waves through LDS + __popcll of
 * the ballot below the lane).  Validity is loaded by bytes only (see the
 * hazard note in DESIGN.md).  Value slots of null rows are never read.
 * Plain stores in a fixed order; nothing depends on the grid size. */
__global__ __launch_bounds__(ENC_PREP_THREADS) void k_enc_prepare(
    const EncGroupCol *__restrict__ cols, int ncols,
    const EncPageSpec *__restrict__ pages, int npages,
    int32_t *__restrict__ cnt, GsPageInfo *__restrict__ info) {
    __shared__ int32_t wcnt[ENC_PREP_WAVES];
    __shared__ uint64_t smin[ENC_PREP_WAVES], smax[ENC_PREP_WAVES];
    __shared__ int32_t sminr[ENC_PREP_WAVES], smaxr[ENC_PREP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nwork = ncols * npages;
    for (int w = blockIdx.x; w < nwork; w += gridDim.x) {
        const int c = w / npages, p = w - c * npages;
        const EncGroupCol col = cols[c];
        const EncPageSpec ps = pages[p];
        const int ct = col.ctype;
        const bool is_bool = ct == GS_CT_BOOL;
        const int32_t n = ps.nrows;
        const int32_t bl = (n + 7) / 8;
        uint8_t *bs = col.out + int64_t(p) * col.cap + 16;
        const uint8_t *vd = col.valid ? col.valid + ps.row_off : nullptr;
        const uint64_t *v8 = (const uint64_t *)col.vals + ps.row_off;
        const uint8_t *v1 = (const uint8_t *)col.vals + ps.row_off;

        uint64_t mn, mx;
        if (ct == GS_CT_F64) {
            mn = 0x7FEFFFFFFFFFFFFFULL; /* DBL_MAX */
            mx = 0xFFEFFFFFFFFFFFFFULL; /* -DBL_MAX */
        } else if (ct == GS_CT_U64) {
            mn = ~0ULL;
            mx = 0;
        } else {
            mn = 0x7FFFFFFFFFFFFFFFULL; /* INT64_MAX */
            mx = 0x8000000000000000ULL; /* INT64_MIN */
        }
        int32_t mnr = INT32_MAX, mxr = INT32_MAX;

        int32_t carry = 0; /* valid rows before this step */
        for (int32_t base = 0; base < n; base += ENC_PREP_THREADS) {
            const int32_t r = base + int32_t(threadIdx.x);
            const bool v = r < n && (!vd || vd[r] != 0);
            const uint64_t b = __ballot(v);
            if (lane < 8) {
                int32_t bi = (base >> 3) + wave * 8 + lane;
                if (bi < bl) bs[bi] = uint8_t(b >> (8 * lane));
            }
            uint64_t x = 0;
            if (v && !is_bool) x = v8[r];
            if (v && is_bool && vd) x = v1[r];
            if (v && !is_bool) {
                enc_min_merge(ct, mn, mnr, x, r);
                enc_max_merge(ct, mx, mxr, x, r);
            }
            if (vd) { /* same for the whole block */
                if (lane == 0) wcnt[wave] = __popcll(b);
                __syncthreads();
                int32_t pos = carry, tot = 0;
                for (int k = 0; k < ENC_PREP_WAVES; k++) {
                    if (k < wave) pos += wcnt[k];
                    tot += wcnt[k];
                }
                pos += __popcll(b & ((1ULL << lane) - 1));
                if (v) {
                    if (is_bool)
                        ((uint8_t *)col.dense)[ps.row_off + pos] = uint8_t(x);
                    else
                        ((uint64_t *)col.dense)[ps.row_off + pos] = x;
                }
                carry += tot;
                __syncthreads(); /* wcnt is rewritten by the next step */
            }
        }
        const int32_t nn = vd ? carry : n; /* non-null rows */

        if (!is_bool) {
            for (int o = 32; o > 0; o >>= 1) {
                uint64_t ob = __shfl_xor(mn, o);
                int32_t orow = __shfl_xor(mnr, o);
                enc_min_merge(ct, mn, mnr, ob, orow);
                ob = __shfl_xor(mx, o);
                orow = __shfl_xor(mxr, o);
                enc_max_merge(ct, mx, mxr, ob, orow);
            }
            if (lane == 0) {
                smin[wave] = mn; sminr[wave] = mnr;
                smax[wave] = mx; smaxr[wave] = mxr;
            }
        }
        __syncthreads(); /* also: this block's dense stores are visible */
        if (threadIdx.x == 0) {
            if (is_bool) {
                mn = mx = 0;
            } else {
                for (int k = 1; k < ENC_PREP_WAVES; k++) {
                    enc_min_merge(ct, mn, mnr, smin[k], sminr[k]);
                    enc_max_merge(ct, mx, mxr, smax[k], smaxr[k]);
                }
            }
            cnt[w] = nn;
            info[w].null_count = int64_t(n) - nn;
            info[w].min_bits = mn;
            info[w].max_bits = mx;
        }
        if (is_bool && nn > 0) {
            /* the bool block (gs_tsm_enc.h): thread 0 writes the header,
               every thread its share of the bit area, one output byte from
               8 dense bytes at a time */
            const uint8_t *src = vd ? (const uint8_t *)col.dense + ps.row_off : v1;
            uint8_t *data = bs + bl;
            if (threadIdx.x == 0) tsm_bool_header(data, uint64_t(nn));
            uint8_t *bits = data + tsm_bool_header_len(uint64_t(nn));
            const int32_t nb = (nn + 7) / 8;
            for (int32_t j = threadIdx.x; j < nb; j += ENC_PREP_THREADS)
                bits[j] = tsm_bool_byte(src, size_t(nn), size_t(j));
        }
        __syncthreads(); /* smin.. are rewritten by the next work item */
    }
}

/* one thread per (column, page): encode the dense values and seal the
 * page */
__global__ void k_enc_group_pages(const EncGroupCol *__restrict__ cols,
                                  int ncols,
                                  const EncPageSpec *__restrict__ pages,
                                  int npages, const int32_t *__restrict__ cnt,
                                  GsPageInfo *__restrict__ info,
                                  unsigned *__restrict__ err) {
    __shared__ uint32_t crct[256];
    enc_crc_table(crct);
    const int nwork = ncols * npages;
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < nwork;
         w += gridDim.x * blockDim.x) {
        const int c = w / npages, p = w - c * npages;
        const EncGroupCol col = cols[c];
        const EncPageSpec ps = pages[p];
        uint8_t *pg = col.out + int64_t(p) * col.cap;
        const uint32_t bl = uint32_t(ps.nrows + 7) / 8;
        uint8_t *data = pg + 16 + bl;
        const int32_t nn = cnt[w];
        if ((col.ctype == GS_CT_TIME || (col.flags & ENC_COL_NO_NULLS)) &&
            nn != ps.nrows) {
            atomicOr(err, DERR_ENC_NULL); /* the time column is never null */
            info[w].len = -3;
            continue;
        }
        const void *src = col.dense ? col.dense : col.vals;
        int64_t dl;
        if (col.ctype == GS_CT_F64)
            dl = tsm_enc_gorilla((const double *)src + ps.row_off, size_t(nn),
                                 data);
        else if (col.ctype == GS_CT_BOOL) /* packed by k_enc_prepare */
            dl = int64_t(tsm_bool_len(uint64_t(nn)));
        else /* u64 is the i64 codec over the same bits (unsigned.rs:15-18) */
            dl = tsm_enc_int(col.ctype == GS_CT_TIME,
                             (const int64_t *)src + ps.row_off, size_t(nn),
                             data, nullptr);
        info[w].len = enc_seal_page(pg, bl, ps.nrows, data, dl, crct, err);
    }
}

/* ---- string page re-encode (gs_encode_str_pages_dev): the pages of one
 * string column, Arrow varbinary in HBM, as host.str_page_of writes them.
 * The block encoder is gs_str_enc.h, the source gs_encode_str runs.  Two
 * launches, one wave per page in both: k_str_enc_measure sizes each page's
 * payload and checks its offsets, the host lays out one payload slab per
 * page, and k_str_enc_pages builds bitset and payload with the whole wave
 * and then lets lane 0 run the snappy match search, which is sequential by
 * definition, so parallelism is pages in flight (as in k_str_decode and
 * k_enc_group_pages).  Bytes of null rows are never read. */

struct StrEncMeasure {
    int64_t payload; /* sum(len + varint_len(len)) over the non-null rows */
    int32_t nn;      /* non-null rows */
    int32_t bad;     /* an offset decreases inside the page */
};

#define STR_ENC_THREADS 64
/* strings up to this long are copied by their own lane, longer ones by the
 * whole wave, one string at a time */
#define STR_ENC_LANE_COPY 32

__global__ __launch_bounds__(STR_ENC_THREADS) void k_str_enc_measure(
    const int64_t *__restrict__ off, const uint8_t *__restrict__ valid,
    const EncPageSpec *__restrict__ pages, int npages,
    StrEncMeasure *__restrict__ out) {
    const int lane = threadIdx.x;
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        const EncPageSpec ps = pages[p];
        const int64_t *o = off + ps.row_off;
        const uint8_t *vd = valid ? valid + ps.row_off : nullptr;
        int64_t payload = 0;
        int32_t nn = 0, bad = 0;
        for (int32_t r = lane; r < ps.nrows; r += STR_ENC_THREADS) {
            const int64_t len = o[r + 1] - o[r];
            if (len < 0) { bad = 1; continue; }
            if (!vd || vd[r] != 0) {
                nn++;
                payload += len + int64_t(tsm_varint_len(uint64_t(len)));
            }
        }
        for (int s = 32; s > 0; s >>= 1) {
            payload += __shfl_xor(payload, s);
            nn += __shfl_xor(nn, s);
            bad |= __shfl_xor(bad, s);
        }
        if (lane == 0) {
            out[p].payload = payload;
            out[p].nn = nn;
            out[p].bad = bad;
        }
    }
}

/* a < b as unsigned bytes, a proper prefix smaller (Rust slice Ord) */
__device__ __forceinline__ int str_enc_cmp(const uint8_t *a, int64_t na,
                                           const uint8_t *b, int64_t nb) {
    const int64_t n = na < nb ? na : nb;
    for (int64_t i = 0; i < n; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return na < nb ? -1 : na > nb ? 1 : 0;
}

/* (value, row) under "smaller value, then smaller row" is a total order, so
 * the minimum is the same row for any partition of the rows; likewise
 * "larger value, then smaller row" for the maximum.  Rows are page-relative,
 * -1 = none. */
__device__ __forceinline__ int str_enc_row_cmp(const int64_t *o,
                                               const uint8_t *bytes, int32_t a,
                                               int32_t b) {
    return str_enc_cmp(bytes + o[a], o[a + 1] - o[a], bytes + o[b],
                       o[b + 1] - o[b]);
}
__device__ __forceinline__ void str_enc_min_merge(const int64_t *o,
                                                  const uint8_t *bytes,
                                                  int32_t &m, int32_t r) {
    if (r < 0) return;
    if (m < 0) { m = r; return; }
    const int c = str_enc_row_cmp(o, bytes, r, m);
    if (c < 0 || (c == 0 && r < m)) m = r;
}
__device__ __forceinline__ void str_enc_max_merge(const int64_t *o,
                                                  const uint8_t *bytes,
                                                  int32_t &m, int32_t r) {
    if (r < 0) return;
    if (m < 0) { m = r; return; }
    const int c = str_enc_row_cmp(o, bytes, r, m);
    if (c > 0 || (c == 0 && r < m)) m = r;
}

/* One wave per page.  Per 64-row step the __ballot of the validity bytes is
 * 8 bytes of the LSB-first bitset (validity loaded by bytes, as in
 * k_enc_prepare), and a wave prefix sum of len + varint_len(len) over the
 * non-null rows gives every string its place in the page's payload slab.
 * Lane 0 then compresses the slab fragment by fragment, straight into the
 * page, through the LDS hash table the wave zeroes for it; the same LDS
 * holds the CRC table afterwards. */
__global__ __launch_bounds__(STR_ENC_THREADS) void k_str_enc_pages(
    const int64_t *__restrict__ off, const uint8_t *__restrict__ bytes,
    const uint8_t *__restrict__ valid, const EncPageSpec *__restrict__ pages,
    int npages, const int64_t *__restrict__ slab_off,
    uint8_t *__restrict__ slabs, uint8_t *__restrict__ out, int64_t cap,
    GsPageInfo *__restrict__ info, unsigned *__restrict__ err) {
    __shared__ uint16_t tab[STR_ENC_MAX_TABLE];
    const int lane = threadIdx.x;
    for (int p = blockIdx.x; p < npages; p += gridDim.x) {
        const EncPageSpec ps = pages[p];
        const int32_t n = ps.nrows;
        const int32_t bl = (n + 7) / 8;
        const int64_t *o = off + ps.row_off;
        const uint8_t *vd = valid ? valid + ps.row_off : nullptr;
        uint8_t *pg = out + int64_t(p) * cap;
        uint8_t *bs = pg + 16;
        uint8_t *data = bs + bl;
        uint8_t *slab = slabs + slab_off[p];

        int64_t carry = 0; /* payload bytes before this step */
        int32_t nn = 0, mnr = -1, mxr = -1;
        for (int32_t base = 0; base < n; base += STR_ENC_THREADS) {
            const int32_t r = base + lane;
            const bool v = r < n && (!vd || vd[r] != 0);
            const uint64_t b = __ballot(v);
            if (lane < 8) {
                const int32_t bi = (base >> 3) + lane;
                if (bi < bl) bs[bi] = uint8_t(b >> (8 * lane));
            }
            nn += __popcll(b);
            int64_t src = 0, len = 0, sz = 0;
            if (v) {
                src = o[r];
                len = o[r + 1] - src;
                sz = len + int64_t(tsm_varint_len(uint64_t(len)));
            }
            int64_t incl = sz;
            for (int s = 1; s < 64; s <<= 1) {
                const int64_t u = __shfl_up(incl, s);
                if (lane >= s) incl += u;
            }
            int64_t dst = carry + incl - len; /* the string's bytes */
            if (v) {
                tsm_varint_put(slab + dst - (sz - len), uint64_t(len));
                if (len <= STR_ENC_LANE_COPY)
                    str_enc_copy(slab + dst, bytes + src, size_t(len));
                str_enc_min_merge(o, bytes, mnr, r);
                str_enc_max_merge(o, bytes, mxr, r);
            }
            uint64_t big = __ballot(v && len > STR_ENC_LANE_COPY);
            while (big) {
                const int l = __builtin_ctzll(big);
                big &= big - 1;
                const int64_t bsrc = __shfl(src, l), blen = __shfl(len, l);
                const int64_t bdst = __shfl(dst, l);
                for (int64_t i = lane; i < blen; i += STR_ENC_THREADS)
                    slab[bdst + i] = bytes[bsrc + i];
            }
            carry += __shfl(incl, 63);
        }
        for (int s = 32; s > 0; s >>= 1) {
            str_enc_min_merge(o, bytes, mnr, __shfl_xor(mnr, s));
            str_enc_max_merge(o, bytes, mxr, __shfl_xor(mxr, s));
        }
        const int64_t payload = carry;

        /* the slab is written by all lanes and read by lane 0 */
        __threadfence();
        __syncthreads();
        int64_t dl = 0;
        if (payload > 0) {
            if (lane == 0) dl = int64_t(str_enc_block_header(data, uint64_t(payload)));
            for (int64_t fo = 0; fo < payload; fo += STR_ENC_FRAGMENT) {
                const size_t frag = payload - fo < int64_t(STR_ENC_FRAGMENT)
                                        ? size_t(payload - fo)
                                        : size_t(STR_ENC_FRAGMENT);
                const uint32_t tsz = str_enc_table_size(frag);
                for (uint32_t i = lane; i < tsz; i += STR_ENC_THREADS) tab[i] = 0;
                __syncthreads();
                if (lane == 0)
                    dl = str_enc_fragment(slab + fo, frag, data + dl, tab) - data;
                __syncthreads();
            }
        }
        /* the hash table's LDS now holds the CRC table */
        uint32_t *crct = (uint32_t *)tab;
        enc_crc_table(crct);
        if (lane == 0) {
            info[p].len = enc_seal_page(pg, uint32_t(bl), n, data, dl, crct, err);
            info[p].null_count = int64_t(n) - nn;
            info[p].min_bits = mnr < 0 ? ~0ULL : uint64_t(ps.row_off + mnr);
            info[p].max_bits = mxr < 0 ? ~0ULL : uint64_t(ps.row_off + mxr);
        }
        __syncthreads(); /* tab is zeroed again by the next page */
    }
}

/* ------------------------------------------- column-group filter kernels
 * gs_filter_group: DataFilter over a column group (reader/filter.rs:91-142)
 * behind decode_pages' tombstones (tsm/reader.rs:494-560).  Every term of
 * the keep rule is a function of one row, so the work item is a stretch of
 * the set's ROW SPACE, not a group: every block does the same amount of work
 * whatever the page size or the series count (k_rle_ts_tiles against
 * k_rle_ts_filtered).  A wave owns FLT_SEG consecutive rows and walks them
 * 64 at a time, a block of four waves a tile of FLT_TILE rows, and the
 * kept count is kept PER WAVE SEGMENT: after the two-level scan over the
 * segment counts each wave of the gather knows where its rows go, so
 * neither kernel has LDS or a block barrier.  A kept row's rank inside the
 * segment is popcount(ballot below the lane) plus the wave's running count
 * of the steps before (the wave carry).  The cell rules are gs_filter.h's. */
#define FLT_SEG 512                /* rows per wave: 8 steps of 64 */
#define FLT_TILE (4 * FLT_SEG)     /* rows per 256-thread block */

struct FltCol {              /* one column as the kernels see it */
    const void *val;         /* 8 B/row, bool 1 B/row; unused for strings */
    const uint8_t *valid;    /* NULL = all valid */
    void *out_val;           /* gather; a string column's reference array */
    uint8_t *out_valid;      /* gather; may be NULL */
    int32_t rng_off;         /* this column's slice of the range table */
    int32_t rng_cnt;
    int32_t ctype;           /* GS_CT_* */
    int32_t pad;
};

struct FltMaskArgs {
    const int64_t *ts;
    const GsTimeRange *ranges; /* normalised lists; the row tombstones first */
    int64_t rows;
    int64_t lo, hi;
    int32_t row_rng_cnt;
    int32_t npreds;
    GsColPred pred[GS_MAX_FILTER_PREDS];
    FltCol pcol[GS_MAX_FILTER_PREDS]; /* the column of pred[p] */
};

struct FltGatherArgs {
    const int64_t *ts;
    const GsTimeRange *ranges;
    int64_t rows;
    int32_t ncol;            /* projected columns only */
    int32_t pad;
    FltCol col[GS_MAX_MERGE_COLS];
};

__device__ __forceinline__ bool flt_effective(const FltCol &c,
                                              const GsTimeRange *ranges,
                                              int64_t r, int64_t t) {
    if (c.valid && !c.valid[r]) return false; /* byte loads only */
    return !(c.rng_cnt && flt_in_ranges(ranges + c.rng_off, c.rng_cnt, t));
}

/* the keep rule of row r with timestamp t: the time range, the row
   tombstones and the conjunction (gs_filter_group and gs_agg_group) */
__device__ __forceinline__ bool flt_keep(const FltMaskArgs &a, int64_t r,
                                         int64_t t) {
    bool keep = t >= a.lo && t <= a.hi &&
                !(a.row_rng_cnt && flt_in_ranges(a.ranges, a.row_rng_cnt, t));
    for (int p = 0; p < a.npreds; p++) {
        if (!keep) break;
        const FltCol &c = a.pcol[p];
        const int op = a.pred[p].op;
        const bool ev = flt_effective(c, a.ranges, r, t);
        uint64_t x = 0;
        if (ev && !flt_op_is_null_test(op))
            x = c.ctype == GS_CT_BOOL ? uint64_t(((const uint8_t *)c.val)[r])
                                      : ((const uint64_t *)c.val)[r];
        keep = flt_cell(op, c.ctype, a.pred[p].a_bits, a.pred[p].b_bits, x,
                        ev);
    }
    return keep;
}

/* mask[r] = the keep rule; seg_cnt[seg] = kept rows of the wave's segment */
__global__ __launch_bounds__(256) void k_flt_mask(
    FltMaskArgs a, int64_t nseg, uint8_t *__restrict__ mask,
    int64_t *__restrict__ seg_cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntile = (nseg + 3) / 4;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t seg = tile * 4 + wave;
        if (seg >= nseg) continue; /* wave-uniform; no barrier below */
        int cnt = 0;
        for (int s = 0; s < FLT_SEG / 64; s++) {
            const int64_t r = seg * FLT_SEG + s * 64 + lane;
            bool keep = false;
            if (r < a.rows) {
                keep = flt_keep(a, r, a.ts[r]);
                mask[r] = keep;
            }
            cnt += __popcll(__ballot(keep));
        }
        if (lane == 0) seg_cnt[seg] = cnt;
    }
}

/* kept rows to their output rows: timestamp, then value and validity of
 * every projected column, 8-byte and 1-byte columns in the same launch, an
 * effectively null cell as zero bytes.  A string column is an 8-byte column
 * whose cell is the reference k_cm_str_lens / k_cm_str_gather take:
 * 1 + row (stream 0), 0 for a null cell. */
__global__ __launch_bounds__(256) void k_flt_gather(
    FltGatherArgs a, int64_t nseg, const uint8_t *__restrict__ mask,
    const int64_t *__restrict__ seg_off, int64_t *__restrict__ out_ts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t ntile = (nseg + 3) / 4;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t seg = tile * 4 + wave;
        if (seg >= nseg) continue;
        int64_t base = seg_off[seg]; /* + the wave carry, step by step */
        for (int s = 0; s < FLT_SEG / 64; s++) {
            const int64_t r = seg * FLT_SEG + s * 64 + lane;
            const bool m = r < a.rows && mask[r];
            const uint64_t b = __ballot(m);
            if (!b) continue;
            if (m) {
                const int64_t pos =
                    base + __builtin_amdgcn_mbcnt_hi(
                               uint32_t(b >> 32),
                               __builtin_amdgcn_mbcnt_lo(uint32_t(b), 0u));
                const int64_t t = a.ts[r];
                out_ts[pos] = t;
                for (int k = 0; k < a.ncol; k++) {
                    const FltCol &c = a.col[k];
                    const bool ev = flt_effective(c, a.ranges, r, t);
                    if (c.out_valid) c.out_valid[pos] = ev;
                    if (c.ctype == GS_CT_STR)
                        ((uint64_t *)c.out_val)[pos] = ev ? uint64_t(r) + 1 : 0;
                    else if (c.ctype == GS_CT_BOOL)
                        ((uint8_t *)c.out_val)[pos] =
                            ev ? ((const uint8_t *)c.val)[r] : uint8_t(0);
                    else
                        ((uint64_t *)c.out_val)[pos] =
                            ev ? ((const uint64_t *)c.val)[r] : 0;
                }
            }
            base += __popcll(b);
        }
    }
}

/* out_off[g] = output row at which group g's rows start (g == ng: the
 * total): the prefix of the group's first row's segment plus the kept rows
 * of that segment in front of the row.  One wave per group. */
__global__ void k_flt_group_off(const DevGroup *__restrict__ groups, int ng,
                                int64_t rows, const uint8_t *__restrict__ mask,
                                const int64_t *__restrict__ seg_off,
                                int64_t nseg, int64_t *__restrict__ out_off) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t(gridDim.x) * blockDim.x) >> 6;
    for (int64_t g = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
         g <= ng; g += nw) {
        const int64_t r0 = g < ng ? groups[g].row_off : rows;
        int64_t v;
        if (r0 >= rows) {
            v = seg_off[nseg];
        } else {
            const int64_t seg = r0 / FLT_SEG;
            int c = 0;
            for (int64_t r = seg * FLT_SEG + lane; r < r0; r += 64)
                c += mask[r];
            for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
            v = seg_off[seg] + c;
        }
        if (lane == 0) out_off[g] = v;
    }
}

/* --------------------------------------- column-group aggregate kernels
 * gs_agg_group: the keep rule of gs_filter_group, reduced straight into
 * (series, bucket) cells.  Rows of a series are contiguous, series ascend
 * along the row space and buckets along a sorted series, so the cell KEY
 * series * n_buckets + slot (agg_bucket's slot: a row in no bucket sorts
 * next to the bucket beside it and contributes nothing) never decreases and
 * every cell is ONE run of consecutive rows.  The work item is the filter's
 * wave segment of FLT_SEG rows, whatever the series or bucket sizes:
 *
 *   k_agg_init     the empty-cell values into every requested array
 *   k_agg_seg      pass A, once per segment: timestamp, keep rule, series,
 *                  slot and key of every row, and the sorted check; pass B,
 *                  once per aggregated column: a segmented reduction over
 *                  the runs of the segment.  While whole 64-row steps stay
 *                  inside the open run each lane folds its own rows and no
 *                  lane talks to another; a step in which the key changes is
 *                  folded by a segmented scan over the lanes (run heads =
 *                  "key differs from the lane before").  Runs that begin
 *                  and end inside the segment are written to their cell; the
 *                  first and the last run go to the segment's two carry
 *                  records
 *   k_agg_stitch   one wave per (run of equal carry keys, column): folds
 *                  the records of a run that crosses segments, however many,
 *                  and writes its cell
 *   k_agg_fold     per_series == 0 only: the (series, bucket) partials are
 *                  kept whole in scratch and one wave per (bucket, column)
 *                  folds them over the series
 *
 * No value is ever added atomically and nothing depends on which block ran
 * first: which rows meet in which fold is fixed by the segment geometry
 * alone, so an f64 sum has the same bits under any grid.  agg_combine is
 * commutative by its row indices (gs_agg.h), which is what lets a lane fold
 * rows 64 apart and a butterfly fold the lanes.  Pass A keeps its per-row
 * results in LDS as a lane-private array (no barrier: no lane reads
 * another's slot), so pass B is one compact loop, not eight unrolled
 * copies. */
struct AggCol {              /* one aggregated column; ctype GS_CT_TIME and
                                val NULL: the kept-row counter (d_rows) */
    FltCol c;
    int64_t *o_count;
    uint64_t *o_sum, *o_mn, *o_mx, *o_first, *o_last;
    int64_t *o_first_ts, *o_last_ts;
};

struct AggGeom {
    const DevGroup *sg;      /* series-level groups */
    int32_t nsg;
    int32_t nb;
    int64_t t0, bn;
    int32_t ncol;            /* aggregated columns (+ 1 for d_rows) */
    int32_t pad;
    uint64_t *scratch;       /* per_series == 0: [ncol][AGG_NFIELD][scells] */
    int64_t scells;          /* nsg * nb */
    int64_t *ckey;           /* [nrec] carry keys: 2 * seg head, + 1 tail */
    uint64_t *ctab;          /* [ncol][AGG_NFIELD][nrec] carry partials */
    int64_t nrec;
};

__device__ __forceinline__ uint64_t agg_shfl64(uint64_t v, int src) {
    const uint32_t lo = __shfl(uint32_t(v), src, 64);
    const uint32_t hi = __shfl(uint32_t(v >> 32), src, 64);
    return (uint64_t(hi) << 32) | lo;
}

__device__ __forceinline__ AggPart agg_shfl(const AggPart &p, int src) {
    uint64_t w[AGG_NFIELD];
    __builtin_memcpy(w, &p, sizeof(AggPart));
#pragma unroll
    for (int f = 0; f < AGG_NFIELD; f++) w[f] = agg_shfl64(w[f], src);
    AggPart o;
    __builtin_memcpy(&o, w, sizeof(AggPart));
    return o;
}

/* fold over the 64 lanes; every lane ends with the same bits */
__device__ __forceinline__ AggPart agg_wave_fold(int ct, AggPart p, int lane) {
    for (int off = 32; off > 0; off >>= 1)
        p = agg_combine(ct, p, agg_shfl(p, lane ^ off));
    return p;
}

__device__ __forceinline__ void agg_tab_store(uint64_t *tab, int64_t n, int k,
                                              int64_t i, const AggPart &p) {
    uint64_t w[AGG_NFIELD];
    __builtin_memcpy(w, &p, sizeof(AggPart));
#pragma unroll
    for (int f = 0; f < AGG_NFIELD; f++)
        tab[(int64_t(k) * AGG_NFIELD + f) * n + i] = w[f];
}

__device__ __forceinline__ AggPart agg_tab_load(const uint64_t *tab, int64_t n,
                                                int k, int64_t i) {
    uint64_t w[AGG_NFIELD];
#pragma unroll
    for (int f = 0; f < AGG_NFIELD; f++)
        w[f] = tab[(int64_t(k) * AGG_NFIELD + f) * n + i];
    AggPart o;
    __builtin_memcpy(&o, w, sizeof(AggPart));
    return o;
}

/* a finished cell into the caller's arrays */
__device__ __forceinline__ void agg_write_out(const AggCol &c, int64_t cell,
                                              const AggPart &p) {
    if (c.o_count) c.o_count[cell] = p.count;
    if (c.o_sum) c.o_sum[cell] = p.sum;
    if (c.o_mn) c.o_mn[cell] = p.mn;
    if (c.o_mx) c.o_mx[cell] = p.mx;
    if (c.o_first) c.o_first[cell] = p.first;
    if (c.o_last) c.o_last[cell] = p.last;
    if (c.o_first_ts) c.o_first_ts[cell] = p.first_ts;
    if (c.o_last_ts) c.o_last_ts[cell] = p.last_ts;
}

/* a finished (series, bucket) run: to the caller's arrays, or whole into the
   scratch that k_agg_fold reduces over the series */
__device__ __forceinline__ void agg_emit(const AggGeom &g, const AggCol &c,
                                         int k, int64_t key, const AggPart &p) {
    if (g.scratch)
        agg_tab_store(g.scratch, g.scells, k, key, p);
    else
        agg_write_out(c, key, p);
}

/* the last series in [lo, hi) that starts at or before row r; series without
   rows share their start with the next one that has some, which is the last
   of them, so the answer always holds r.  Needs sg[lo].row_off <= r. */
__device__ __forceinline__ int agg_series_of(const DevGroup *sg, int lo, int hi,
                                             int64_t r) {
    while (hi - lo > 1) {
        const int m = lo + ((hi - lo) >> 1);
        if (sg[m].row_off <= r) lo = m; else hi = m;
    }
    return lo;
}

__global__ void k_agg_init(AggGeom g, const AggCol *__restrict__ cols,
                           int64_t ncell) {
    const int64_t n = g.scratch ? g.scells : ncell;
    const int64_t step = int64_t(gridDim.x) * blockDim.x;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n;
         i += step)
        for (int k = 0; k < g.ncol; k++)
            agg_emit(g, cols[k], k, i, agg_empty(cols[k].c.ctype));
}

__global__ __launch_bounds__(256) void k_agg_seg(
    FltMaskArgs a, AggGeom g, const AggCol *__restrict__ cols, int64_t nseg,
    unsigned *__restrict__ err) {
    /* lane-private [step][thread]: no lane reads another's slot */
    __shared__ int64_t s_ts[FLT_SEG / 64][256];
    __shared__ int64_t s_key[FLT_SEG / 64][256];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int64_t ntile = (nseg + 3) / 4;
    for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        const int64_t seg = tile * 4 + wave;
        if (seg >= nseg) continue; /* wave-uniform; no barrier below */
        const int64_t r0 = seg * FLT_SEG;
        const int64_t left = a.rows - r0; /* >= 1 */
        const int nstep = left >= FLT_SEG ? FLT_SEG / 64 : int((left + 63) >> 6);

        /* ---- pass A: every row's timestamp, key and "contributes" bit.
           Lanes behind the last row repeat it and contribute nothing. */
        uint32_t cbits = 0;
        int s_cur = __builtin_amdgcn_readfirstlane(
            agg_series_of(g.sg, 0, g.nsg, r0));
        bool w_ok = false; /* bucket window of the last row of the step before */
        uint64_t w_lo = 0, w_b = 0;
        int64_t prev63 = r0 > 0 ? a.ts[r0 - 1] : 0;
        for (int s = 0; s < nstep; s++) {
            const int64_t r = r0 + s * 64 + lane;
            const bool in = r < a.rows;
            const int64_t rc = in ? r : a.rows - 1;
            const int64_t r_hi = r0 + s * 64 + 63 < a.rows ? r0 + s * 64 + 63
                                                           : a.rows - 1;
            const int64_t t = a.ts[rc];
            /* series: from the table only in a step a boundary falls in */
            int ser = s_cur;
            if (s_cur + 1 < g.nsg && g.sg[s_cur + 1].row_off <= r_hi) {
                int hi = s_cur + 65 < g.nsg ? s_cur + 65 : g.nsg;
                if (hi < g.nsg && g.sg[hi].row_off <= r_hi) hi = g.nsg;
                ser = agg_series_of(g.sg, s_cur, hi, rc);
            }
            s_cur = __builtin_amdgcn_readlane(ser, 63);
            /* sorted inside the series: a compare with the row before */
            const int64_t up =
                int64_t(agg_shfl64(uint64_t(t), lane ? lane - 1 : 0));
            const int64_t prev = lane ? up : prev63;
            if (in && r > g.sg[ser].row_off && t <= prev)
                atomicOr(err, DERR_NONMONO);
            prev63 = int64_t(agg_shfl64(uint64_t(t), 63));
            /* bucket: the window carried from the step before answers for
               the same and the next bucket; only other rows divide */
            uint64_t b = 0;
            bool before = false;
            if (g.bn != 0) {
                before = t < g.t0;
                const uint64_t d = uint64_t(t) - uint64_t(g.t0);
                if (!before &&
                    !(w_ok && agg_bucket_near(d, w_lo, w_b, uint64_t(g.bn), &b)))
                    agg_bucket_raw(t, g.t0, g.bn, &b);
            }
            int32_t slot = 0;
            const bool inb = !before && agg_slot(b, g.nb, &slot);
            w_ok = g.bn != 0 && !__shfl(int(before), 63, 64);
            w_b = agg_shfl64(b, 63);
            w_lo = w_b * uint64_t(g.bn); /* <= ts - t0: no overflow */
            s_ts[s][tid] = t;
            s_key[s][tid] = int64_t(ser) * g.nb + slot;
            if (in && inb && flt_keep(a, r, t)) cbits |= 1u << s;
        }

        /* ---- pass B: column by column over the stored steps */
        const int64_t key_first = agg_shfl64(uint64_t(s_key[0][tid]), 0);
        for (int k = 0; k < g.ncol; k++) {
            const AggCol col = cols[k];
            const int ct = col.c.ctype;
            AggPart acc = agg_empty(ct);  /* this lane's rows of the open run */
            AggPart open = agg_empty(ct); /* the open run before those */
            int64_t open_key = key_first;
            bool open_is_first = true;
            for (int s = 0; s < nstep; s++) {
                const int64_t r = r0 + s * 64 + lane;
                const int64_t t = s_ts[s][tid];
                const int64_t key = s_key[s][tid];
                AggPart me = agg_empty(ct);
                if ((cbits >> s) & 1) {
                    if (!col.c.val) {
                        me = agg_single(ct, 0, t, r);
                    } else if (flt_effective(col.c, a.ranges, r, t)) {
                        const uint64_t x =
                            ct == GS_CT_BOOL
                                ? uint64_t(((const uint8_t *)col.c.val)[r])
                                : ((const uint64_t *)col.c.val)[r];
                        me = agg_single(ct, x, t, r);
                    }
                }
                const int64_t k0 = agg_shfl64(uint64_t(key), 0);
                const int64_t k63 = agg_shfl64(uint64_t(key), 63);
                if (k0 == open_key && k63 == open_key) { /* wave-uniform */
                    acc = agg_combine(ct, acc, me);
                    continue;
                }
                /* the key changes in this step: segmented inclusive scan */
                AggPart sc = me;
                for (int off = 1; off < 64; off <<= 1) {
                    const int src = lane >= off ? lane - off : lane;
                    const AggPart o = agg_shfl(sc, src);
                    const int64_t ko = agg_shfl64(uint64_t(key), src);
                    if (lane >= off && ko == key) sc = agg_combine(ct, o, sc);
                }
                /* close the open run: what came before, the lanes' own rows,
                   and the leading lanes of this step that still belong to it */
                AggPart tot = agg_combine(ct, open, agg_wave_fold(ct, acc, lane));
                const int p = __popcll(__ballot(key == open_key));
                if (p > 0) tot = agg_combine(ct, tot, agg_shfl(sc, p - 1));
                if (lane == 0) {
                    if (open_is_first) {
                        g.ckey[2 * seg] = open_key;
                        agg_tab_store(g.ctab, g.nrec, k, 2 * seg, tot);
                    } else {
                        agg_emit(g, col, k, open_key, tot);
                    }
                }
                open_is_first = false;
                /* runs that end inside this step and are not the open one */
                const int nxt = lane < 63 ? lane + 1 : lane;
                const int64_t kn = agg_shfl64(uint64_t(key), nxt);
                if (lane < 63 && kn != key && key != open_key)
                    agg_emit(g, col, k, key, sc);
                /* the run that reaches the step's end is the open one now */
                open = agg_shfl(sc, 63);
                open_key = k63;
                acc = agg_empty(ct);
            }
            const AggPart tot =
                agg_combine(ct, open, agg_wave_fold(ct, acc, lane));
            if (lane == 0) {
                /* one run over the whole segment: the tail record is the
                   same key with nothing in it */
                g.ckey[2 * seg + 1] = open_key;
                if (open_is_first) {
                    g.ckey[2 * seg] = open_key;
                    agg_tab_store(g.ctab, g.nrec, k, 2 * seg, tot);
                    agg_tab_store(g.ctab, g.nrec, k, 2 * seg + 1,
                                  agg_empty(ct));
                } else {
                    agg_tab_store(g.ctab, g.nrec, k, 2 * seg + 1, tot);
                }
            }
        }
    }
}

/* Carry keys never decrease, so the records of one cell are consecutive.
   One wave per (record that starts a run of equal keys, column): the lanes
   fold records 64 apart, a butterfly folds the lanes, lane 0 writes the
   cell.  The shape of the fold depends on the run alone. */
__global__ __launch_bounds__(256) void k_agg_stitch(
    AggGeom g, const AggCol *__restrict__ cols) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const int64_t items = g.nrec * g.ncol;
    for (int64_t it = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
         it < items; it += nw) {
        const int64_t rec = it / g.ncol;
        const int k = int(it - rec * g.ncol);
        const int64_t key = g.ckey[rec];
        if (rec > 0 && g.ckey[rec - 1] == key) continue; /* wave-uniform */
        const AggCol col = cols[k];
        const int ct = col.c.ctype;
        AggPart acc = agg_empty(ct);
        for (int64_t i = rec + lane; i < g.nrec && g.ckey[i] == key; i += 64)
            acc = agg_combine(ct, acc, agg_tab_load(g.ctab, g.nrec, k, i));
        acc = agg_wave_fold(ct, acc, lane);
        if (lane == 0) agg_emit(g, col, k, key, acc);
    }
}

/* per_series == 0: cell b of column k = the fold of scratch cells
   (s, b) over the series, one wave per (bucket, column) */
__global__ __launch_bounds__(256) void k_agg_fold(
    AggGeom g, const AggCol *__restrict__ cols) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t(gridDim.x) * blockDim.x) >> 6;
    const int64_t items = int64_t(g.nb) * g.ncol;
    for (int64_t it = (blockIdx.x * int64_t(blockDim.x) + threadIdx.x) >> 6;
         it < items; it += nw) {
        const int64_t b = it / g.ncol;
        const int k = int(it - b * g.ncol);
        const AggCol col = cols[k];
        const int ct = col.c.ctype;
        AggPart acc = agg_empty(ct);
        for (int64_t s = lane; s < g.nsg; s += 64)
            acc = agg_combine(ct, acc, agg_tab_load(g.scratch, g.scells, k,
                                                    s * g.nb + b));
        acc = agg_wave_fold(ct, acc, lane);
        if (lane == 0) agg_write_out(col, b, acc);
    }
}

/* ------------------------------------------------------------- host state */

struct GsCtx {
    int device;
    hipStream_t stream;
    unsigned *d_err;
};

/* Every capped launch takes its grid from grid_for or grid_items, so one
   debug override (gs_debug_set_grid_cap) can drive any kernel through
   several trips of its grid-stride loop on a set of a few thousand pages.
   g_grid_cap <= 0: no override.  g_grid_rounds: the largest
   ceil(uncapped blocks / granted blocks) seen since the last reset. */
static std::atomic<int> g_grid_cap{0};
static std::atomic<int> g_grid_rounds{0};

/* one item per block: min(items, the site's cap), block-stride beyond */
static int grid_items(int64_t want, int cap) {
    int64_t g = want > cap ? cap : want;
    int dbg = g_grid_cap.load(std::memory_order_relaxed);
    if (dbg > 0 && g > dbg) g = dbg;
    if (g > 0) {
        int64_t trips = (want + g - 1) / g;
        int r = trips > INT32_MAX ? INT32_MAX : int(trips);
        int seen = g_grid_rounds.load(std::memory_order_relaxed);
        while (r > seen && !g_grid_rounds.compare_exchange_weak(
                               seen, r, std::memory_order_relaxed)) {
        }
    }
    return int(g);
}

/* one item per thread (or per per_block-thread block): at most 2048 blocks,
   grid-stride beyond (Guideline 11) */
static int grid_for(int64_t work, int per_block) {
    int64_t want = (work + per_block - 1) / per_block;
    return grid_items(want < 1 ? 1 : want, 2048);
}

struct SlotPages {
    uint8_t ctype;
    std::vector<DevPage> host[PC_NCLASS];
    DevPage *dev[PC_NCLASS] = {nullptr, nullptr, nullptr};
    int n[PC_NCLASS] = {0, 0, 0};
    /* string pages only: per-PC_STR-page scratch offsets (host order of
       host[PC_STR]) + total; caps parsed from the block headers at
       upload (snappy preamble varint / uncompressed payload length) */
    std::vector<int64_t> str_scr;
    uint64_t str_total = 0;
    int64_t *d_str_scr = nullptr;
    /* Gorilla chunk table (page-major over host[PC_GOR]; states filled by
       the k_gor_sync upload pre-pass) */
    DevGorChunk *d_gor_chunks = nullptr;
    int n_gor_chunks = 0;
    int32_t *d_gor_chunk_base = nullptr; /* [n[PC_GOR]+1] */
    DevGorChunk *d_gorn_chunks = nullptr;
    int n_gorn_chunks = 0;
    int32_t *d_gorn_chunk_base = nullptr; /* [n[PC_GORN]+1] */
    /* fused aggregate (PC_GOR): DevGorChunk.slot ordinal of each
       page-group's first chunk, and from it the series groups' slot
       ranges.  agg_fused_ok: every page-group has exactly one PC_GOR page
       in this slot and every chunk a slot, so a series group's pieces are
       one contiguous, time-ordered slot range. */
    std::vector<int32_t> gor_grp_cbase;  /* [ngroups+1] */
    int32_t *d_sg_chunk_first = nullptr; /* [nsgroups+1] */
    int max_sg_chunks = 0;
    bool agg_fused_ok = false;
};

/* fused-scan phase events (scan_fused_launch / scan_fused_wait) */
enum { SEV_START, SEV_OFFS, SEV_TS, SEV_VAL, SEV_END, GS_NSEV };

struct GsGroupSet {
    GsCtx *ctx = nullptr;
    uint8_t *d_blob = nullptr;
    size_t blob_len = 0;
    int64_t total_rows = 0;
    size_t ngroups = 0;
    uint32_t ncols = 0;
    std::vector<int64_t> row_offsets;
    std::vector<SlotPages> slots;
    DevGroup *d_groups = nullptr;
    DevGroup *d_sgroups = nullptr; /* series-level (consecutive same-series
                                      groups merged) for aggregation */
    int nsgroups = 0;
    std::vector<int32_t> sgroup_span; /* page-groups per series-group */
    std::vector<int64_t> sgroup_row_off; /* first row of each series-group */
    DevGroup *d_sgroups_out = nullptr; /* series-group layout of the fused
                                          compacted output (rebuilt per scan) */
    int32_t *d_sgroup_first = nullptr; /* [nsgroups+1] first page-group idx */
    int64_t *d_blocksums = nullptr;    /* device-scan scratch */
    hipEvent_t sev[GS_NSEV];           /* fused-scan phase events */
    bool sev_init = false;
    bool pending = false;              /* an async fused scan is in flight */
    int64_t *d_sp_start = nullptr;
    int64_t *d_sp_cnt = nullptr;
    int64_t *d_out_off = nullptr;
    int64_t *d_g_t0sel = nullptr; /* per page-group: ts of first selected
                                     row / RLE delta (k_spans_rle out) */
    int64_t *d_g_delta = nullptr;
    int max_span = 0; /* max page-groups per series-group */
    /* fused-scan active-chunk list (lazy; sized to the largest slot's
       chunk table) */
    int *d_gor_active = nullptr;
    int *d_gor_nactive = nullptr;
    size_t gor_active_cap = 0;
    /* fused aggregate: page-group -> series group, the per-chunk head/tail
       pieces (lazy; two per chunk of the largest slot, reused from field
       to field like the partial cells), and the smallest positive RLE
       delta of the time pages (INT64_MAX if none) for the gate */
    int32_t *d_grp_sgroup = nullptr;
    DevAggMeta *d_agg_meta = nullptr;
    DevAggVal *d_agg_val = nullptr;
    size_t agg_pieces_cap = 0;
    int64_t min_pos_delta = INT64_MAX;
    /* string decode scratch (lazy, cached across gs_decode_str calls) */
    uint8_t *d_str_scratch = nullptr;
    size_t str_scratch_cap = 0;
    int64_t *d_str_sz = nullptr;  /* per-row string byte length (0=null) */
    int64_t *d_str_pos = nullptr; /* per-row start index into scratch */
    int64_t *d_str_bsums = nullptr; /* offset-scan block sums over rows */
    size_t str_bsums_cap = 0;
    GsTimeRange *d_ranges = nullptr;
    size_t ranges_cap = 0;
    uint8_t *d_valid = nullptr; /* lazily allocated internal validity bytes */
    uint8_t *d_mask = nullptr;  /* value-predicate row mask (lazy) */
    /* gs_filter_group scratch (lazy, cached across calls): per-segment kept
       counts, their prefix and the scan's block sums in one block; the
       normalised range lists; the string reference columns and lengths */
    int64_t *d_flt_seg = nullptr;
    GsTimeRange *d_flt_ranges = nullptr;
    size_t flt_ranges_cap = 0;
    uint64_t *d_flt_ref = nullptr;
    size_t flt_ref_cap = 0;
    /* gs_agg_group scratch (lazy, cached across calls, sizes in 8-byte
       words): the segments' carry keys and partials; the column table; the
       (series, bucket) partials of a per_series == 0 call */
    uint64_t *d_agg_carry = nullptr;
    size_t agg_carry_cap = 0;
    void *d_agg_cols = nullptr;
    uint64_t *d_agg_scr = nullptr;
    size_t agg_scr_cap = 0;
    int64_t *d_sel_cnt = nullptr; /* per-group masked selected counts (lazy) */
    bool any_nulls_field = false;
    /* agg partials: ngroups x nbuckets cells, cached across scans */
    double *d_pmax = nullptr;
    double *d_psum = nullptr;
    long long *d_pcnt = nullptr;
    size_t partials_cap = 0;
};

extern "C" {

int gs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

GsCtx *gs_ctx_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
        fail(GS_ERR_NO_GPU, "no HIP device available — cnosdb_gs has no CPU fallback");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        fail(GS_ERR, "device index out of range");
        return nullptr;
    }
    HIP_TRY_NULL(hipSetDevice(device));
    GsCtx *ctx = new GsCtx();
    ctx->device = device;
    if (hipStreamCreate(&ctx->stream) != hipSuccess ||
        hipMalloc(&ctx->d_err, sizeof(unsigned)) != hipSuccess) {
        fail(GS_ERR, "ctx init failed");
        delete ctx;
        return nullptr;
    }
    hipMemset(ctx->d_err, 0, sizeof(unsigned));
    return ctx;
}

void gs_ctx_destroy(GsCtx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    hipFree(ctx->d_err);
    hipStreamDestroy(ctx->stream);
    delete ctx;
}

GsGroupSet *gs_groups_upload(GsCtx *ctx, const GsColumnGroupDesc *groups,
                             size_t ngroups, int validate_crc) {
    if (!ctx || !groups || ngroups == 0) {
        fail(GS_ERR, "bad args to gs_groups_upload");
        return nullptr;
    }
    HIP_TRY_NULL(hipSetDevice(ctx->device));
    uint32_t ncols = groups[0].npages;
    for (size_t g = 0; g < ngroups; g++) {
        if (groups[g].npages != ncols || ncols == 0) {
            fail(GS_ERR, "all groups must have the same page schema");
            return nullptr;
        }
        if (groups[g].pages[0].ctype != GS_CT_TIME) {
            fail(GS_ERR, "pages[0] of every group must be the time page");
            return nullptr;
        }
    }

    GsGroupSet *set = new GsGroupSet();
    set->ctx = ctx;
    set->ngroups = ngroups;
    set->ncols = ncols;
    set->slots.resize(ncols);
    set->row_offsets.resize(ngroups);

    /* pass 1: layout + validation + classification */
    struct HostPage {
        const uint8_t *bitset_src;
        const uint8_t *data_src;
        uint32_t bitset_len;
        uint32_t col;
        DevPage dp;
    };
    std::vector<HostPage> staged;
    staged.reserve(ngroups * ncols);
    size_t blob = 0;
    int64_t rows = 0;
    auto align16 = [](size_t x) { return (x + 15) & ~size_t(15); };
    for (size_t g = 0; g < ngroups; g++) {
        set->row_offsets[g] = rows;
        uint32_t nrows_g = groups[g].pages[0].num_values;
        for (uint32_t c = 0; c < ncols; c++) {
            const GsPageSpec &ps = groups[g].pages[c];
            if (ps.len < 16) { fail(GS_ERR_FORMAT, "page too short"); gs_groups_free(set); return nullptr; }
            uint32_t bl = (uint32_t(ps.bytes[0]) << 24) | (uint32_t(ps.bytes[1]) << 16) |
                          (uint32_t(ps.bytes[2]) << 8) | ps.bytes[3];
            uint64_t dl64 = 0;
            for (int k = 0; k < 8; k++) dl64 = (dl64 << 8) | ps.bytes[4 + k];
            if (16ull + bl > ps.len) { fail(GS_ERR_FORMAT, "bitset overruns page"); gs_groups_free(set); return nullptr; }
            if (dl64 != ps.num_values || ps.num_values != nrows_g) {
                fail(GS_ERR_FORMAT, "row count mismatch in group");
                gs_groups_free(set); return nullptr;
            }
            uint64_t data_len = ps.len - 16 - bl;
            const uint8_t *bitset = ps.bytes + 16;
            const uint8_t *data = ps.bytes + 16 + bl;
            if (validate_crc) {
                uint32_t crc = (uint32_t(ps.bytes[12]) << 24) | (uint32_t(ps.bytes[13]) << 16) |
                               (uint32_t(ps.bytes[14]) << 8) | ps.bytes[15];
                if (gs_crc32(data, data_len) != crc) {
                    fail(GS_ERR_CRC, "page crc32 mismatch");
                    gs_groups_free(set); return nullptr;
                }
            }
            /* all_valid: full bytes 0xff, partial last byte has low bits set */
            bool av = true;
            uint32_t full = ps.num_values / 8, restbits = ps.num_values % 8;
            if (bl * 8 < ps.num_values) av = false;
            else {
                for (uint32_t k = 0; k < full; k++)
                    if (bitset[k] != 0xff) { av = false; break; }
                if (av && restbits) {
                    uint8_t mask = uint8_t((1u << restbits) - 1);
                    if ((bitset[full] & mask) != mask) av = false;
                }
            }
            HostPage hp;
            hp.bitset_src = bitset;
            hp.data_src = data;
            hp.bitset_len = bl;
            hp.col = c;
            hp.dp.bitset_off = blob;
            blob += bl;
            blob = align16(blob);
            hp.dp.data_off = blob;
            blob += data_len;
            blob = align16(blob);
            blob += 48; /* tail pad: the Gorilla fast path prefetches whole
                           words up to ~32 B past the data end (guarded by
                           its bit budget, garbage never interpreted) */
            hp.dp.row_off = rows;
            hp.dp.data_len = uint32_t(data_len);
            hp.dp.nrows = ps.num_values;
            hp.dp.ctype = ps.ctype;
            hp.dp.enc = data_len ? data[0] : 0;
            hp.dp.sub = uint8_t(
                int_page_header(data, uint32_t(data_len), hp.dp.enc).sub);
            hp.dp.all_valid = av ? 1 : 0;
            hp.dp.grp = uint32_t(g);
            if (c == 0 && !av) {
                fail(GS_ERR_FORMAT, "time page must be fully valid");
                gs_groups_free(set); return nullptr;
            }
            if (c > 0 && !av) set->any_nulls_field = true;
            staged.push_back(hp);
        }
        rows += nrows_g;
    }
    set->total_rows = rows;
    set->blob_len = blob;

    /* allocate + upload blob through chunked pinned staging (double-
     * buffered; the pages sit in arbitrary user memory, so per-page
     * hipMemcpyAsync would cost ~4 us apiece — 246k copies measured) */
    if (hipMalloc(&set->d_blob, blob ? blob : 16) != hipSuccess) {
        fail(GS_ERR, "hipMalloc blob failed (out of HBM?)");
        gs_groups_free(set); return nullptr;
    }
    {
        const size_t CHUNK = size_t(256) << 20;
        uint8_t *stage[2] = {nullptr, nullptr};
        hipEvent_t evs[2];
        for (int k = 0; k < 2; k++) {
            if (hipHostMalloc(&stage[k], CHUNK) != hipSuccess) {
                fail(GS_ERR, "hipHostMalloc staging failed");
                gs_groups_free(set); return nullptr;
            }
            hipEventCreate(&evs[k]);
            hipEventRecord(evs[k], ctx->stream);
        }
        int cur = 0;
        size_t base = 0, fill_end = 0;
        size_t pi = 0;
        while (pi < staged.size()) {
            hipEventSynchronize(evs[cur]);
            base = staged[pi].dp.bitset_off;
            fill_end = base;
            size_t start_pi = pi;
            while (pi < staged.size()) {
                const HostPage &hp = staged[pi];
                size_t page_end = hp.dp.data_off + hp.dp.data_len;
                if (page_end - base > CHUNK) break;
                memcpy(stage[cur] + (hp.dp.bitset_off - base), hp.bitset_src,
                       hp.bitset_len);
                if (hp.dp.data_len)
                    memcpy(stage[cur] + (hp.dp.data_off - base), hp.data_src,
                           hp.dp.data_len);
                fill_end = page_end;
                pi++;
            }
            if (pi == start_pi) { /* single page larger than CHUNK */
                fail(GS_ERR, "page larger than staging chunk");
                for (int k = 0; k < 2; k++) { hipHostFree(stage[k]); hipEventDestroy(evs[k]); }
                gs_groups_free(set); return nullptr;
            }
            hipMemcpyAsync(set->d_blob + base, stage[cur], fill_end - base,
                           hipMemcpyHostToDevice, ctx->stream);
            hipEventRecord(evs[cur], ctx->stream);
            cur ^= 1;
        }
        hipStreamSynchronize(ctx->stream);
        for (int k = 0; k < 2; k++) { hipHostFree(stage[k]); hipEventDestroy(evs[k]); }
    }

    /* classify + upload page tables */
    for (uint32_t c = 0; c < ncols; c++) set->slots[c].ctype = 255;
    for (auto &hp : staged) {
        SlotPages &sp = set->slots[hp.col];
        if (sp.ctype == 255) sp.ctype = hp.dp.ctype;
        if (hp.dp.ctype != sp.ctype) {
            fail(GS_ERR, "mixed ctypes in one column slot");
            gs_groups_free(set); return nullptr;
        }
        int cls = PC_SEQ;
        bool int_ct = hp.dp.ctype == GS_CT_TIME || hp.dp.ctype == GS_CT_I64 ||
                      hp.dp.ctype == GS_CT_U64;
        if (hp.dp.ctype == GS_CT_STR) {
            cls = PC_STR;
            /* scratch slab: decoded payload length (snappy preamble
               varint, string.rs:197, capped by what the stream can
               produce) or the raw payload (Null enc) */
            sp.str_scr.push_back(int64_t(sp.str_total));
            sp.str_total += str_slab_stride(
                str_slab_size(hp.data_src, hp.dp.data_len, hp.dp.enc));
        } else if (hp.dp.all_valid && hp.dp.sub == 2 && int_ct && hp.dp.data_len > 2) {
            if (hp.dp.enc == GS_ENC_DELTATS) cls = PC_RLE_TS;
            else if (hp.dp.enc == GS_ENC_DELTA) cls = PC_RLE_I64;
            if (cls == PC_RLE_TS && hp.col == 0) {
                /* RLE delta as k_spans_rle reads it; a page it refuses
                   contributes nothing */
                const IntHeader h = int_page_header(
                    hp.data_src, hp.dp.data_len, hp.dp.enc);
                if (!h.verdict && h.rle_delta > 0 &&
                    h.rle_delta < set->min_pos_delta)
                    set->min_pos_delta = h.rle_delta;
            }
        } else if (hp.dp.all_valid && hp.dp.sub == 1 && int_ct &&
                   (hp.dp.enc == GS_ENC_DELTATS || hp.dp.enc == GS_ENC_DELTA) &&
                   hp.dp.data_len > 2) {
            cls = PC_S8B;
        } else if (hp.dp.enc == GS_ENC_GORILLA &&
                   hp.dp.ctype == GS_CT_F64 && hp.dp.data_len >= 10) {
            cls = hp.dp.all_valid ? PC_GOR : PC_GORN;
        } else if (hp.dp.all_valid && hp.dp.enc == GS_ENC_NULL &&
                   hp.dp.ctype != GS_CT_BOOL && hp.dp.data_len >= 1) {
            cls = PC_RAW;
        } else if (hp.dp.all_valid && hp.dp.enc == GS_ENC_BITPACK &&
                   hp.dp.ctype == GS_CT_BOOL && hp.dp.data_len >= 3) {
            cls = PC_BOOL;
        }
        sp.host[cls].push_back(hp.dp);
    }
    for (uint32_t c = 0; c < ncols; c++) {
        SlotPages &sp = set->slots[c];
        /* longest Gorilla pages first: decode time scales with compressed
           bits, so launching the slow pages early removes the ragged tail */
        std::stable_sort(sp.host[PC_GOR].begin(), sp.host[PC_GOR].end(),
                         [](const DevPage &a, const DevPage &b) {
                             return a.data_len > b.data_len;
                         });
        for (int k = 0; k < PC_NCLASS; k++) {
            sp.n[k] = int(sp.host[k].size());
            if (sp.n[k]) {
                if (hipMalloc(&sp.dev[k], sp.n[k] * sizeof(DevPage)) != hipSuccess) {
                    fail(GS_ERR, "hipMalloc page table failed");
                    gs_groups_free(set); return nullptr;
                }
                hipMemcpyAsync(sp.dev[k], sp.host[k].data(),
                               sp.n[k] * sizeof(DevPage),
                               hipMemcpyHostToDevice, ctx->stream);
            }
        }
        if (sp.n[PC_STR]) {
            if (hipMalloc(&sp.d_str_scr, sp.n[PC_STR] * sizeof(int64_t)) != hipSuccess) {
                fail(GS_ERR, "hipMalloc str scratch table failed");
                gs_groups_free(set); return nullptr;
            }
            hipMemcpyAsync(sp.d_str_scr, sp.str_scr.data(),
                           sp.n[PC_STR] * sizeof(int64_t),
                           hipMemcpyHostToDevice, ctx->stream);
        }
        for (int gcls = 0; gcls < 2; gcls++) {
            /* chunk skeletons (page-major) for the two Gorilla classes,
               states filled by k_gor_sync / k_gor_sync_null.  Chunk size
               is tunable for sweeps (GS_GOR_CHUNK env). */
            const int pc = gcls == 0 ? PC_GOR : PC_GORN;
            if (!sp.n[pc]) continue;
            static uint32_t chunk_rows = [] {
                const char *e = getenv("GS_GOR_CHUNK");
                long v = e ? atol(e) : 0;
                return uint32_t(v >= 64 ? v : GOR_CHUNK);
            }();
            std::vector<int32_t> cbase(sp.n[pc] + 1);
            std::vector<DevGorChunk> hch;
            int32_t acc = 0;
            auto nch_of = [&](const DevPage &pg) {
                return pg.nrows ? (pg.nrows + chunk_rows - 1) / chunk_rows
                                : 1u;
            };
            if (gcls == 0) {
                /* chunk ordinals in page-group order (the table below is
                   sorted by page length): DevGorChunk.slot */
                sp.gor_grp_cbase.assign(ngroups + 1, 0);
                for (int i = 0; i < sp.n[pc]; i++)
                    sp.gor_grp_cbase[sp.host[pc][i].grp + 1] +=
                        int32_t(nch_of(sp.host[pc][i]));
                for (size_t g = 0; g < ngroups; g++)
                    sp.gor_grp_cbase[g + 1] += sp.gor_grp_cbase[g];
                sp.agg_fused_ok = sp.n[pc] == int(ngroups);
            }
            for (int i = 0; i < sp.n[pc]; i++) {
                const DevPage &pg = sp.host[pc][i];
                cbase[i] = acc;
                uint32_t nch = nch_of(pg);
                for (uint32_t k = 0; k < nch; k++) {
                    DevGorChunk c{};
                    c.data_off = pg.data_off;
                    c.bitset_off = pg.bitset_off;
                    c.row_off = pg.row_off;
                    c.grp = pg.grp;
                    c.row0 = k * chunk_rows;
                    c.cnt = pg.nrows > c.row0
                                ? (pg.nrows - c.row0 < chunk_rows
                                       ? pg.nrows - c.row0 : chunk_rows)
                                : 0;
                    c.data_len = pg.data_len;
                    c.meaningful = 64;
                    c.last = uint8_t(k == nch - 1);
                    c.slot = gcls == 0
                                 ? uint32_t(sp.gor_grp_cbase[pg.grp]) + k
                                 : GOR_NO_SLOT;
                    hch.push_back(c);
                }
                acc += int32_t(nch);
            }
            cbase[sp.n[pc]] = acc;
            DevGorChunk **dchp = gcls == 0 ? &sp.d_gor_chunks
                                           : &sp.d_gorn_chunks;
            int32_t **dcbp = gcls == 0 ? &sp.d_gor_chunk_base
                                       : &sp.d_gorn_chunk_base;
            (gcls == 0 ? sp.n_gor_chunks : sp.n_gorn_chunks) = acc;
            if (hipMalloc(dchp, hch.size() * sizeof(DevGorChunk)) !=
                    hipSuccess ||
                hipMalloc(dcbp, cbase.size() * sizeof(int32_t)) !=
                    hipSuccess) {
                fail(GS_ERR, "hipMalloc gor chunk table failed");
                gs_groups_free(set); return nullptr;
            }
            hipMemcpyAsync(*dchp, hch.data(),
                           hch.size() * sizeof(DevGorChunk),
                           hipMemcpyHostToDevice, ctx->stream);
            hipMemcpyAsync(*dcbp, cbase.data(),
                           cbase.size() * sizeof(int32_t),
                           hipMemcpyHostToDevice, ctx->stream);
            /* hch/cbase are stack-local: wait for the staged copies before
               they go out of scope (upload path, not scan time) */
            hipStreamSynchronize(ctx->stream);
            /* one-time sync-point pre-pass (upload/setup, not scan time) */
            if (gcls == 0)
                hipLaunchKernelGGL(k_gor_sync,
                                   dim3(grid_for(sp.n[pc], 256)), dim3(256),
                                   0, ctx->stream, set->d_blob, sp.dev[pc],
                                   sp.n[pc], *dcbp, *dchp, chunk_rows);
            else
                hipLaunchKernelGGL(k_gor_sync_null,
                                   dim3(grid_for(sp.n[pc], 256)), dim3(256),
                                   0, ctx->stream, set->d_blob, sp.dev[pc],
                                   sp.n[pc], *dcbp, *dchp, chunk_rows);
        }
    }

    /* group table + span scratch */
    std::vector<DevGroup> hg(ngroups);
    for (size_t g = 0; g < ngroups; g++) {
        hg[g].row_off = set->row_offsets[g];
        hg[g].nrows = int32_t(groups[g].pages[0].num_values);
        hg[g].pad = 0;
    }
    /* series-level groups: merge consecutive page-groups of one series
       (their rows are contiguous and time-ordered) */
    std::vector<DevGroup> hsg;
    for (size_t g = 0; g < ngroups; g++) {
        if (!hsg.empty() && g > 0 &&
            groups[g].series_id == groups[g - 1].series_id) {
            hsg.back().nrows += hg[g].nrows;
            set->sgroup_span.back()++;
        } else {
            hsg.push_back(hg[g]);
            set->sgroup_span.push_back(1);
            set->sgroup_row_off.push_back(hg[g].row_off);
        }
    }
    set->nsgroups = int(hsg.size());
    if (hipMalloc(&set->d_sgroups, hsg.size() * sizeof(DevGroup)) != hipSuccess) {
        fail(GS_ERR, "hipMalloc sgroup table failed");
        gs_groups_free(set); return nullptr;
    }
    hipMemcpyAsync(set->d_sgroups, hsg.data(), hsg.size() * sizeof(DevGroup),
                   hipMemcpyHostToDevice, ctx->stream);
    size_t nblocks = (ngroups + SCAN_BLOCK * SCAN_ITEMS - 1) /
                     (SCAN_BLOCK * SCAN_ITEMS);
    std::vector<int32_t> sgfirst(hsg.size() + 1);
    {
        int32_t acc32 = 0;
        for (size_t s = 0; s < hsg.size(); s++) {
            sgfirst[s] = acc32;
            acc32 += set->sgroup_span[s];
        }
        sgfirst[hsg.size()] = acc32;
    }
    if (hipMalloc(&set->d_groups, ngroups * sizeof(DevGroup)) != hipSuccess ||
        hipMalloc(&set->d_sp_start, ngroups * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_sp_cnt, ngroups * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_out_off, (ngroups + 1) * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_blocksums, (nblocks + 1) * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_sgroup_first, sgfirst.size() * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&set->d_sgroups_out, hsg.size() * sizeof(DevGroup)) != hipSuccess ||
        hipMalloc(&set->d_g_t0sel, ngroups * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_g_delta, ngroups * sizeof(int64_t)) != hipSuccess) {
        fail(GS_ERR, "hipMalloc group tables failed");
        gs_groups_free(set); return nullptr;
    }
    for (int32_t sp : set->sgroup_span)
        if (sp > set->max_span) set->max_span = sp;
    hipMemcpyAsync(set->d_sgroup_first, sgfirst.data(),
                   sgfirst.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                   ctx->stream);
    hipMemcpyAsync(set->d_groups, hg.data(), ngroups * sizeof(DevGroup),
                   hipMemcpyHostToDevice, ctx->stream);
    /* fused-aggregate tables: page-group -> series group, and per Gorilla
       slot the series groups' ranges of chunk ordinals.  Page-groups of a
       series group are consecutive and the ordinals run in page-group
       order, so each range is contiguous by construction; checked anyway,
       and a slot that fails keeps the separate aggregate kernel. */
    std::vector<int32_t> grp_sg(ngroups);
    for (size_t s = 0; s < hsg.size(); s++)
        for (int32_t g = sgfirst[s]; g < sgfirst[s + 1]; g++)
            grp_sg[g] = int32_t(s);
    std::vector<std::vector<int32_t>> sgc(ncols);
    if (hipMalloc(&set->d_grp_sgroup, ngroups * sizeof(int32_t)) != hipSuccess) {
        fail(GS_ERR, "hipMalloc group->sgroup table failed");
        gs_groups_free(set); return nullptr;
    }
    hipMemcpyAsync(set->d_grp_sgroup, grp_sg.data(),
                   ngroups * sizeof(int32_t), hipMemcpyHostToDevice,
                   ctx->stream);
    for (uint32_t c = 0; c < ncols; c++) {
        SlotPages &sp = set->slots[c];
        if (!sp.agg_fused_ok) continue;
        std::vector<int32_t> &t = sgc[c];
        t.resize(hsg.size() + 1);
        for (size_t s = 0; s <= hsg.size(); s++)
            t[s] = sp.gor_grp_cbase[sgfirst[s]];
        /* (the ordinals number exactly the table's chunks) */
        if (t[0] != 0 || t[hsg.size()] > sp.n_gor_chunks)
            sp.agg_fused_ok = false;
        for (size_t s = 0; s < hsg.size() && sp.agg_fused_ok; s++) {
            if (t[s + 1] < t[s]) sp.agg_fused_ok = false;
            if (t[s + 1] - t[s] > sp.max_sg_chunks)
                sp.max_sg_chunks = t[s + 1] - t[s];
        }
        if (!sp.agg_fused_ok) continue;
        if (hipMalloc(&sp.d_sg_chunk_first, t.size() * sizeof(int32_t)) != hipSuccess) {
            fail(GS_ERR, "hipMalloc sgroup chunk table failed");
            gs_groups_free(set); return nullptr;
        }
        hipMemcpyAsync(sp.d_sg_chunk_first, t.data(),
                       t.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                       ctx->stream);
    }
    HIP_TRY_NULL(hipStreamSynchronize(ctx->stream));
    return set;
}

void gs_groups_free(GsGroupSet *set) {
    if (!set) return;
    hipSetDevice(set->ctx->device);
    hipStreamSynchronize(set->ctx->stream);
    for (auto &sp : set->slots) {
        for (int k = 0; k < PC_NCLASS; k++)
            if (sp.dev[k]) hipFree(sp.dev[k]);
        if (sp.d_str_scr) hipFree(sp.d_str_scr);
        if (sp.d_gor_chunks) hipFree(sp.d_gor_chunks);
        if (sp.d_gor_chunk_base) hipFree(sp.d_gor_chunk_base);
        if (sp.d_gorn_chunks) hipFree(sp.d_gorn_chunks);
        if (sp.d_gorn_chunk_base) hipFree(sp.d_gorn_chunk_base);
        if (sp.d_sg_chunk_first) hipFree(sp.d_sg_chunk_first);
    }
    if (set->d_grp_sgroup) hipFree(set->d_grp_sgroup);
    if (set->d_agg_meta) hipFree(set->d_agg_meta);
    if (set->d_agg_val) hipFree(set->d_agg_val);
    if (set->d_gor_active) hipFree(set->d_gor_active);
    if (set->d_gor_nactive) hipFree(set->d_gor_nactive);
    if (set->d_str_scratch) hipFree(set->d_str_scratch);
    if (set->d_str_sz) hipFree(set->d_str_sz);
    if (set->d_str_pos) hipFree(set->d_str_pos);
    if (set->d_str_bsums) hipFree(set->d_str_bsums);
    hipFree(set->d_blob);
    hipFree(set->d_groups);
    if (set->d_sgroups) hipFree(set->d_sgroups);
    if (set->d_sgroups_out) hipFree(set->d_sgroups_out);
    if (set->d_sgroup_first) hipFree(set->d_sgroup_first);
    if (set->d_blocksums) hipFree(set->d_blocksums);
    if (set->sev_init)
        for (int k = 0; k < GS_NSEV; k++) hipEventDestroy(set->sev[k]);
    hipFree(set->d_sp_start);
    hipFree(set->d_sp_cnt);
    hipFree(set->d_out_off);
    if (set->d_g_t0sel) hipFree(set->d_g_t0sel);
    if (set->d_g_delta) hipFree(set->d_g_delta);
    if (set->d_ranges) hipFree(set->d_ranges);
    if (set->d_valid) hipFree(set->d_valid);
    if (set->d_mask) hipFree(set->d_mask);
    if (set->d_flt_seg) hipFree(set->d_flt_seg);
    if (set->d_flt_ranges) hipFree(set->d_flt_ranges);
    if (set->d_flt_ref) hipFree(set->d_flt_ref);
    if (set->d_agg_carry) hipFree(set->d_agg_carry);
    if (set->d_agg_cols) hipFree(set->d_agg_cols);
    if (set->d_agg_scr) hipFree(set->d_agg_scr);
    if (set->d_sel_cnt) hipFree(set->d_sel_cnt);
    if (set->d_pmax) hipFree(set->d_pmax);
    if (set->d_psum) hipFree(set->d_psum);
    if (set->d_pcnt) hipFree(set->d_pcnt);
    delete set;
}

/* debug: copy a slot's GORN chunk table to host (repro tooling only) */
int64_t gs_debug_gorn_table(GsCtx *ctx, GsGroupSet *set, uint32_t col,
                            DevGorChunk *out, int64_t cap) {
    if (!ctx || !set || col >= set->ncols) return -1;
    SlotPages &sp = set->slots[col];
    int64_t n = sp.n_gorn_chunks;
    if (!out || cap < n) return n;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (hipMemcpy(out, sp.d_gorn_chunks, size_t(n) * sizeof(DevGorChunk),
                  hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return n;
}

int64_t gs_debug_read_blob(GsCtx *ctx, GsGroupSet *set, uint64_t off,
                           uint64_t len, uint8_t *out) {
    if (!ctx || !set || off + len > set->blob_len) return -1;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (hipMemcpy(out, set->d_blob + off, len, hipMemcpyDeviceToHost) !=
        hipSuccess)
        return -1;
    return int64_t(len);
}

int64_t gs_debug_rerun_gorn_sync(GsCtx *ctx, GsGroupSet *set,
                                 uint32_t col) {
    if (!ctx || !set || col >= set->ncols) return -1;
    SlotPages &sp = set->slots[col];
    if (!sp.n[PC_GORN]) return 0;
    hipSetDevice(ctx->device);
    const char *e = getenv("GS_GOR_CHUNK");
    long v = e ? atol(e) : 0;
    uint32_t chunk_rows = uint32_t(v >= 64 ? v : GOR_CHUNK);
    hipLaunchKernelGGL(k_gor_sync_null, dim3(grid_for(sp.n[PC_GORN], 256)),
                       dim3(256), 0, ctx->stream, set->d_blob,
                       sp.dev[PC_GORN], sp.n[PC_GORN], sp.d_gorn_chunk_base,
                       sp.d_gorn_chunks, chunk_rows);
    hipStreamSynchronize(ctx->stream);
    return 1;
}

__global__ void k_debug_crc(const uint8_t *__restrict__ p, uint64_t len,
                            uint64_t *__restrict__ out) {
    /* simple order-independent mix so any byte difference shows */
    uint64_t acc = 0;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < len;
         i += uint64_t(gridDim.x) * blockDim.x)
        acc += (uint64_t(p[i]) + 1) * (i + 0x9e3779b97f4a7c15ULL);
    atomicAdd((unsigned long long *)out, (unsigned long long)acc);
}

int64_t gs_debug_kernel_crc(GsCtx *ctx, GsGroupSet *set, uint64_t off,
                            uint64_t len, uint64_t *out_sum) {
    if (!ctx || !set || off + len > set->blob_len) return -1;
    hipSetDevice(ctx->device);
    uint64_t *d;
    if (hipMalloc(&d, 8) != hipSuccess) return -1;
    hipMemset(d, 0, 8);
    hipLaunchKernelGGL(k_debug_crc, dim3(64), dim3(256), 0, ctx->stream,
                       set->d_blob + off, len, d);
    hipStreamSynchronize(ctx->stream);
    hipMemcpy(out_sum, d, 8, hipMemcpyDeviceToHost);
    hipFree(d);
    return 0;
}

/* debug (test seam): cap every capped launch at max_blocks, so that small
   sets drive the kernels through several trips of their stride loops.
   <= 0 restores the defaults.  Returns the previous setting. */
int32_t gs_debug_set_grid_cap(int32_t max_blocks) {
    return g_grid_cap.exchange(max_blocks > 0 ? max_blocks : 0,
                               std::memory_order_relaxed);
}

/* debug: the largest ceil(uncapped blocks / granted blocks) of any capped
   launch since the last reset */
int32_t gs_debug_grid_rounds(int reset) {
    return reset ? g_grid_rounds.exchange(0, std::memory_order_relaxed)
                 : g_grid_rounds.load(std::memory_order_relaxed);
}

int64_t gs_set_rows(const GsGroupSet *set) { return set ? set->total_rows : -1; }
int64_t gs_set_series(const GsGroupSet *set) { return set ? set->nsgroups : -1; }

/* Pushed-down COUNT answered from page metadata, never from decoded data
 * (PushDownAggregateReader, tskv/src/reader/pushdown_agg_reader.rs:39-106:
 * sums num_values — rows INCLUDING nulls — of the column's pages; SURVEY.md
 * A.10.12). */
int64_t gs_count_pushdown(const GsGroupSet *set, uint32_t col) {
    if (!set || col >= set->ncols) return -1;
    int64_t n = 0;
    const SlotPages &sp = set->slots[col];
    for (int k = 0; k < PC_NCLASS; k++)
        for (const DevPage &p : sp.host[k]) n += p.nrows;
    return n;
}
int64_t gs_set_groups(const GsGroupSet *set) { return set ? int64_t(set->ngroups) : -1; }
GsStatus gs_set_row_offsets(const GsGroupSet *set, int64_t *out) {
    if (!set || !out) return fail(GS_ERR, "bad args");
    memcpy(out, set->row_offsets.data(), set->ngroups * sizeof(int64_t));
    return GS_OK;
}

/* --------------------------------------------- GROUP BY tag
 * TSBS GROUP-BY-hostname over the decoded varbinary tag column.  In the
 * reference a tag is part of the SeriesKey and therefore CONSTANT within
 * a series (tag columns are materialized per series from the key,
 * reader/series.rs:23-100); the GPU group-by exploits exactly that:
 * hash the tag of each series' first row into a device dictionary
 * (first-occurrence = min series index, deterministic), then merge the
 * per-series bucket partials of the preceding aggregate scan per
 * (tag, bucket) in series order — a deterministic fixed-order reduction,
 * like the aggregate itself. */
__device__ __forceinline__ uint64_t dev_fnv1a(const uint8_t *p, int64_t n) {
    uint64_t h = 1469598103934665603ULL;
    for (int64_t i = 0; i < n; i++) {
        h ^= p[i];
        h *= 1099511628211ULL;
    }
    return h;
}

/* dictionary slot, one atomic u64: [fp32 (nonzero) | min_series32].
 * Claim by CAS from 0; equal-tag series then atomicMin the whole word —
 * the high fp bits are equal so the min acts on the series index,
 * keeping the deterministic first-occurrence owner.  fp collisions are
 * resolved by byte comparison against the slot owner's tag (the owner
 * field is valid from the moment the slot exists — single-word claim). */
__global__ void k_tag_series(const DevGroup *__restrict__ sg, int nsg,
                             const int64_t *__restrict__ str_pos,
                             const int64_t *__restrict__ str_sz,
                             const uint8_t *__restrict__ scratch,
                             unsigned long long *__restrict__ table,
                             int cap_mask, int32_t *__restrict__ slot_of,
                             unsigned *__restrict__ err) {
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < nsg;
         g += gridDim.x * blockDim.x) {
        const int64_t r0 = sg[g].row_off; /* tag of the series' first row */
        const uint8_t *tb = scratch + str_pos[r0];
        const int64_t tn = str_sz[r0];
        const uint64_t fphi = (dev_fnv1a(tb, tn) >> 32) | 1ULL;
        const unsigned long long claim =
            (fphi << 32) | (unsigned long long)(uint32_t)g;
        int slot = int(fphi * 0x9e3779b1u) & cap_mask;
        bool placed = false;
        for (int probes = 0; probes <= cap_mask && !placed; probes++) {
            unsigned long long cur = table[slot];
            if (cur == 0) cur = atomicCAS(&table[slot], 0ULL, claim);
            if (cur == 0 || (cur >> 32) == fphi) {
                bool same = true;
                if (cur != 0) { /* verify bytes vs the slot owner */
                    const int own = int(cur & 0xffffffffULL);
                    if (own != g) {
                        const int64_t ro = sg[own].row_off;
                        if (str_sz[ro] != tn) same = false;
                        else {
                            const uint8_t *ob = scratch + str_pos[ro];
                            for (int64_t i = 0; i < tn && same; i++)
                                same = ob[i] == tb[i];
                        }
                    }
                }
                if (same) {
                    atomicMin(&table[slot], claim);
                    slot_of[g] = slot;
                    placed = true;
                    break;
                }
            }
            slot = (slot + 1) & cap_mask;
        }
        if (!placed) atomicOr(err, DERR_FORMAT); /* table full */
    }
}

/* thread per (gid, bucket): ordered walk of the gid's series list */
__global__ void k_agg_tag(const int32_t *__restrict__ csr_off,
                          const int32_t *__restrict__ csr_sg, int ngids,
                          int nbuckets, const double *__restrict__ pmax,
                          const double *__restrict__ psum,
                          const long long *__restrict__ pcnt,
                          double *__restrict__ out_max,
                          double *__restrict__ out_sum,
                          long long *__restrict__ out_cnt) {
    int64_t total = int64_t(ngids) * nbuckets;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x;
         i < total; i += int64_t(gridDim.x) * blockDim.x) {
        const int gid = int(i / nbuckets);
        const int b = int(i % nbuckets);
        double mx = -__builtin_inf(), sm = 0.0;
        long long c = 0;
        for (int32_t k = csr_off[gid]; k < csr_off[gid + 1]; k++) {
            const size_t cell = size_t(csr_sg[k]) * nbuckets + b;
            const long long pc = pcnt[cell];
            if (pc <= 0) continue;
            const double m2 = pmax[cell];
            if (m2 > mx) mx = m2;
            sm += psum[cell];
            c += pc;
        }
        out_max[i] = mx;
        out_sum[i] = sm;
        out_cnt[i] = c;
    }
}

static GsStatus check_dev_err(GsCtx *ctx) {
    unsigned e = 0;
    HIP_TRY(hipMemcpy(&e, ctx->d_err, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (e) {
        hipMemset(ctx->d_err, 0, sizeof(unsigned));
        if (e & DERR_NONMONO)
            return fail(GS_ERR_FORMAT,
                        "decode: non-monotonic time page (corrupt input)");
        if (e & DERR_SHORT) return fail(GS_ERR_FORMAT, "decode: stream shorter than validity demands");
        return fail(GS_ERR_FORMAT, "decode: malformed page data");
    }
    return GS_OK;
}


GsStatus gs_decode(GsCtx *ctx, GsGroupSet *set, uint32_t col, void *d_out,
                   uint8_t *d_valid) {
    if (!ctx || !set || col >= set->ncols || !d_out)
        return fail(GS_ERR, "bad args to gs_decode");
    HIP_TRY(hipSetDevice(ctx->device));
    SlotPages &sp = set->slots[col];
    uint8_t ct = sp.ctype;
    if (sp.n[PC_STR])
        return fail(GS_ERR, "string column: use gs_decode_str");

    if (sp.n[PC_SEQ]) {
        int n = sp.n[PC_SEQ];
        int blocks = grid_for(n, 256);
        if (ct == GS_CT_F64)
            hipLaunchKernelGGL(k_seq_f64, dim3(blocks), dim3(256), 0, ctx->stream,
                               set->d_blob, sp.dev[PC_SEQ], n, (double *)d_out,
                               d_valid, ctx->d_err);
        else if (ct == GS_CT_BOOL)
            hipLaunchKernelGGL(k_seq_bool, dim3(blocks), dim3(256), 0, ctx->stream,
                               set->d_blob, sp.dev[PC_SEQ], n, (uint8_t *)d_out,
                               d_valid, ctx->d_err);
        else
            hipLaunchKernelGGL(k_seq_i64, dim3(blocks), dim3(256), 0, ctx->stream,
                               set->d_blob, sp.dev[PC_SEQ], n, (int64_t *)d_out,
                               d_valid, ctx->d_err);
    }
    if (sp.n[PC_GOR]) {
        int n = sp.n_gor_chunks;
        hipLaunchKernelGGL(k_gor_chunks, dim3(grid_for(n, GS_GOR_BLOCK)),
                           dim3(GS_GOR_BLOCK), 0, ctx->stream, set->d_blob,
                           sp.d_gor_chunks, n, (double *)d_out, ctx->d_err);
        if (d_valid)
            hipLaunchKernelGGL(k_valid_fill,
                               dim3(grid_items(sp.n[PC_GOR], 2048)),
                               dim3(256), 0, ctx->stream, sp.dev[PC_GOR],
                               sp.n[PC_GOR], d_valid);
    }
    if (sp.n[PC_GORN]) {
        int n = sp.n_gorn_chunks;
        hipLaunchKernelGGL(k_gor_chunks_null, dim3(grid_for(n, GS_GOR_BLOCK)),
                           dim3(GS_GOR_BLOCK), 0, ctx->stream, set->d_blob,
                           sp.d_gorn_chunks, n, (double *)d_out, ctx->d_err);
        if (d_valid)
            hipLaunchKernelGGL(
                k_valid_expand,
                dim3(grid_items(sp.n[PC_GORN], 2048)), dim3(256),
                0, ctx->stream, set->d_blob, sp.dev[PC_GORN], sp.n[PC_GORN],
                d_valid);
    }
    if (sp.n[PC_S8B]) {
        int n = sp.n[PC_S8B];
        hipLaunchKernelGGL(k_s8b_par, dim3(grid_items(n, 65535)), dim3(256),
                           0, ctx->stream, set->d_blob, sp.dev[PC_S8B], n,
                           (int64_t *)d_out, d_valid, ctx->d_err);
    }
    if (sp.n[PC_BOOL]) {
        int n = sp.n[PC_BOOL];
        hipLaunchKernelGGL(k_bool_par, dim3(grid_items(n, 65535)), dim3(256),
                           0, ctx->stream, set->d_blob, sp.dev[PC_BOOL], n,
                           (uint8_t *)d_out, d_valid, ctx->d_err);
    }
    if (sp.n[PC_RAW]) {
        int n = sp.n[PC_RAW];
        hipLaunchKernelGGL(k_raw_par, dim3(grid_items(n, 65535)), dim3(256),
                           0, ctx->stream, set->d_blob, sp.dev[PC_RAW], n,
                           (int64_t *)d_out, d_valid, ctx->d_err);
    }
    if (sp.n[PC_RLE_TS])
        hipLaunchKernelGGL(k_rle_par,
                           dim3(grid_items(sp.n[PC_RLE_TS], 2048)),
                           dim3(256), 0, ctx->stream, set->d_blob,
                           sp.dev[PC_RLE_TS], sp.n[PC_RLE_TS], (int64_t *)d_out,
                           d_valid, ctx->d_err);
    if (sp.n[PC_RLE_I64])
        hipLaunchKernelGGL(k_rle_par,
                           dim3(grid_items(sp.n[PC_RLE_I64], 2048)),
                           dim3(256), 0, ctx->stream, set->d_blob,
                           sp.dev[PC_RLE_I64], sp.n[PC_RLE_I64], (int64_t *)d_out,
                           d_valid, ctx->d_err);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return check_dev_err(ctx);
}

/* GROUP BY tag over a completed aggregate scan: the tag column (decoded
 * by gs_decode_str: per-row pos/sz into its scratch) keys a dictionary of
 * the per-series tag (constant within a series, SeriesKey semantics);
 * outputs per-(tag, bucket) max/sum/count in deterministic
 * first-occurrence tag order.  out arrays are caller device buffers of
 * cap_gids * n_buckets; tag_rep_row[gid] (host) = a row whose string is
 * the tag value.  Requires the previous gs_scan on this set to have run
 * with the same n_buckets (the per-series partials are reused). */
GsStatus gs_groupby_tag(GsCtx *ctx, GsGroupSet *set, int tag_col,
                        int n_buckets, double *d_out_max, double *d_out_sum,
                        long long *d_out_count, int64_t *tag_rep_row,
                        int cap_gids, int *out_ngids) {
    if (!ctx || !set || !d_out_max || !d_out_sum || !d_out_count ||
        !out_ngids || n_buckets <= 0)
        return fail(GS_ERR, "bad args to gs_groupby_tag");
    if (!set->d_pmax ||
        set->partials_cap < size_t(set->nsgroups) * size_t(n_buckets))
        return fail(GS_ERR, "gs_groupby_tag needs a prior aggregate scan");
    if (!set->d_str_sz || !set->d_str_pos || !set->d_str_scratch)
        return fail(GS_ERR, "gs_groupby_tag needs a decoded string column");
    (void)tag_col;
    HIP_TRY(hipSetDevice(ctx->device));
    const int nsg = set->nsgroups;
    int cap = 64;
    while (cap < 2 * nsg) cap <<= 1;
    unsigned long long *d_table = nullptr;
    int32_t *d_slot_of = nullptr;
    if (hipMalloc(&d_table, size_t(cap) * 8) != hipSuccess ||
        hipMalloc(&d_slot_of, size_t(nsg) * 4) != hipSuccess) {
        if (d_table) hipFree(d_table);
        return fail(GS_ERR, "hipMalloc tag table failed");
    }
    HIP_TRY(hipMemsetAsync(d_table, 0, size_t(cap) * 8, ctx->stream));
    hipLaunchKernelGGL(k_tag_series, dim3(grid_for(nsg, 256)), dim3(256), 0,
                       ctx->stream, set->d_sgroups, nsg, set->d_str_pos,
                       set->d_str_sz, set->d_str_scratch, d_table, cap - 1,
                       d_slot_of, ctx->d_err);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    GsStatus st = check_dev_err(ctx);
    if (st != GS_OK) { hipFree(d_table); hipFree(d_slot_of); return st; }
    /* host finalize (tiny, deterministic): dense ids in first-occurrence
       order + CSR of the series of each tag */
    std::vector<unsigned long long> table(cap);
    std::vector<int32_t> slot_of(nsg);
    HIP_TRY(hipMemcpy(table.data(), d_table, size_t(cap) * 8,
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(slot_of.data(), d_slot_of, size_t(nsg) * 4,
                      hipMemcpyDeviceToHost));
    hipFree(d_table);
    hipFree(d_slot_of);
    std::vector<std::pair<int, int>> owners; /* (min series, slot) */
    for (int sl = 0; sl < cap; sl++)
        if (table[sl])
            owners.push_back({int(table[sl] & 0xffffffffULL), sl});
    std::sort(owners.begin(), owners.end());
    const int ngids = int(owners.size());
    *out_ngids = ngids;
    if (ngids > cap_gids)
        return fail(GS_ERR, "gs_groupby_tag: cap_gids too small");
    std::vector<int32_t> gid_of_slot(cap, -1);
    for (int gidx = 0; gidx < ngids; gidx++)
        gid_of_slot[owners[gidx].second] = gidx;
    std::vector<int32_t> csr_off(ngids + 1, 0), csr_sg(nsg);
    for (int g = 0; g < nsg; g++) csr_off[gid_of_slot[slot_of[g]] + 1]++;
    for (int gidx = 0; gidx < ngids; gidx++) csr_off[gidx + 1] += csr_off[gidx];
    {
        std::vector<int32_t> cur(csr_off.begin(), csr_off.end() - 1);
        for (int g = 0; g < nsg; g++) /* series order within a tag */
            csr_sg[cur[gid_of_slot[slot_of[g]]]++] = g;
    }
    if (tag_rep_row)
        for (int gidx = 0; gidx < ngids; gidx++) {
            int sgi = owners[gidx].first;
            tag_rep_row[gidx] = size_t(sgi) < set->sgroup_row_off.size()
                                    ? set->sgroup_row_off[sgi] : -1;
        }
    int32_t *d_csr_off = nullptr, *d_csr_sg = nullptr;
    if (hipMalloc(&d_csr_off, (ngids + 1) * 4) != hipSuccess ||
        hipMalloc(&d_csr_sg, size_t(nsg) * 4) != hipSuccess) {
        if (d_csr_off) hipFree(d_csr_off);
        return fail(GS_ERR, "hipMalloc tag csr failed");
    }
    hipMemcpyAsync(d_csr_off, csr_off.data(), (ngids + 1) * 4,
                   hipMemcpyHostToDevice, ctx->stream);
    hipMemcpyAsync(d_csr_sg, csr_sg.data(), size_t(nsg) * 4,
                   hipMemcpyHostToDevice, ctx->stream);
    hipStreamSynchronize(ctx->stream);
    const int64_t total = int64_t(ngids) * n_buckets;
    hipLaunchKernelGGL(k_agg_tag, dim3(grid_for(total, 256)), dim3(256),
                       0, ctx->stream, d_csr_off, d_csr_sg, ngids, n_buckets,
                       set->d_pmax, set->d_psum, set->d_pcnt, d_out_max,
                       d_out_sum, d_out_count);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    hipFree(d_csr_off);
    hipFree(d_csr_sg);
    return check_dev_err(ctx);
}

GsStatus gs_decode_str(GsCtx *ctx, GsGroupSet *set, uint32_t col,
                       int64_t *d_offsets, uint8_t *d_bytes,
                       int64_t bytes_cap, uint8_t *d_valid,
                       int64_t *total_bytes) {
    if (!ctx || !set || col >= set->ncols || !d_offsets || !d_bytes ||
        !total_bytes)
        return fail(GS_ERR, "bad args to gs_decode_str");
    SlotPages &sp = set->slots[col];
    if (sp.ctype != GS_CT_STR || sp.n[PC_STR] != int(sp.host[PC_STR].size()))
        return fail(GS_ERR, "column is not a string column");
    if (set->total_rows > int64_t(SCAN_BLOCK) * SCAN_ITEMS * 131072)
        return fail(GS_ERR, "string decode row limit exceeded (268M)");
    HIP_TRY(hipSetDevice(ctx->device));
    int n = sp.n[PC_STR];
    if (!set->d_str_scratch || set->str_scratch_cap < size_t(sp.str_total)) {
        if (set->d_str_scratch) hipFree(set->d_str_scratch);
        size_t cap = sp.str_total ? size_t(sp.str_total) : 16;
        if (hipMalloc(&set->d_str_scratch, cap) != hipSuccess)
            return fail(GS_ERR, "hipMalloc string scratch failed");
        set->str_scratch_cap = cap;
    }
    if (!set->d_str_sz) {
        if (hipMalloc(&set->d_str_sz, set->total_rows * 8) != hipSuccess ||
            hipMalloc(&set->d_str_pos, set->total_rows * 8) != hipSuccess)
            return fail(GS_ERR, "hipMalloc string row tables failed");
    }
    int nblocks = int((set->total_rows + SCAN_BLOCK * SCAN_ITEMS - 1) /
                      (SCAN_BLOCK * SCAN_ITEMS));
    if (set->str_bsums_cap < size_t(nblocks) + 1) {
        if (set->d_str_bsums) hipFree(set->d_str_bsums);
        if (hipMalloc(&set->d_str_bsums, (size_t(nblocks) + 1) * 8) != hipSuccess)
            return fail(GS_ERR, "hipMalloc string scan sums failed");
        set->str_bsums_cap = size_t(nblocks) + 1;
    }
    hipLaunchKernelGGL(k_str_decode, dim3(grid_for(n, 256)), dim3(256), 0,
                       ctx->stream, set->d_blob, sp.dev[PC_STR], n,
                       sp.d_str_scr, set->d_str_scratch, set->d_str_sz,
                       set->d_str_pos, d_valid, ctx->d_err);
    hipLaunchKernelGGL(k_scan_partials, dim3(nblocks), dim3(SCAN_BLOCK), 0,
                       ctx->stream, set->d_str_sz, int(set->total_rows),
                       d_offsets, set->d_str_bsums);
    hipLaunchKernelGGL(k_scan_fixup, dim3(1), dim3(64), 0, ctx->stream,
                       int(set->total_rows), d_offsets, set->d_str_bsums,
                       nblocks);
    hipLaunchKernelGGL(k_scan_add, dim3(grid_for(int(set->total_rows), 256)),
                       dim3(256), 0, ctx->stream, int(set->total_rows),
                       d_offsets, set->d_str_bsums);
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, d_offsets + set->total_rows, 8,
                           hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    GsStatus st = check_dev_err(ctx);
    if (st != GS_OK) return st;
    if (total > bytes_cap)
        return fail(GS_ERR, "string bytes buffer too small");
    hipLaunchKernelGGL(k_str_gather, dim3(grid_for(int(set->total_rows), 256)),
                       dim3(256), 0, ctx->stream, set->d_str_scratch,
                       set->d_str_pos, set->d_str_sz, d_offsets,
                       set->total_rows, d_bytes);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *total_bytes = total;
    return check_dev_err(ctx);
}

GsStatus gs_apply_tombstone(GsCtx *ctx, GsGroupSet *set, const int64_t *d_ts,
                            uint8_t *d_valid, const GsTimeRange *ranges,
                            size_t nranges) {
    if (!ctx || !set || !d_ts || !d_valid || !ranges || nranges == 0)
        return fail(GS_ERR, "bad args to gs_apply_tombstone");
    HIP_TRY(hipSetDevice(ctx->device));
    if (set->ranges_cap < nranges) {
        if (set->d_ranges) hipFree(set->d_ranges);
        HIP_TRY(hipMalloc(&set->d_ranges, nranges * sizeof(GsTimeRange)));
        set->ranges_cap = nranges;
    }
    HIP_TRY(hipMemcpyAsync(set->d_ranges, ranges, nranges * sizeof(GsTimeRange),
                           hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_tombstone,
                       dim3(grid_items(int64_t(set->ngroups), 2048)),
                       dim3(256), 0, ctx->stream,
                       set->d_groups, int(set->ngroups), d_ts, d_valid,
                       set->d_ranges, int(nranges));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return GS_OK;
}

static bool fused_capable_fields(GsGroupSet *set, const GsScanSpec *spec,
                                 const int32_t *fields, int nf) {
    if (!(spec->d_out_ts && spec->d_out_val && spec->n_tombstones == 0 &&
          spec->value_pred.op == GS_PRED_NONE && !set->any_nulls_field &&
          set->slots[0].n[PC_RLE_TS] == int(set->ngroups)))
        return false;
    for (int f = 0; f < nf; f++) {
        uint32_t fc = 1 + uint32_t(fields[f]);
        if (fc >= set->ncols ||
            set->slots[fc].n[PC_GOR] != int(set->ngroups))
            return false;
    }
    return true;
}

static bool fused_capable(GsGroupSet *set, const GsScanSpec *spec) {
    int32_t f0 = spec->field_col;
    return fused_capable_fields(set, spec, &f0, 1);
}

/* Fused scan over ONE span/ts pass and nf field columns (TSBS
 * cpu-max-all-8, BASELINE config #3: the per-field loop of round 1 paid
 * the span search and the 8 B/row ts generation once PER FIELD).
 * Per-field outputs are strided: field i's compacted values go to
 * d_out_val + i*total_rows; its aggregates to d_agg_* + i*n_buckets. */
static GsStatus scan_fused_launch(GsCtx *ctx, GsGroupSet *set,
                                  const GsScanSpec *spec,
                                  const int32_t *fields, int nf) {
    HIP_TRY(hipSetDevice(ctx->device));
    if (!set->sev_init) {
        for (int k = 0; k < GS_NSEV; k++)
            HIP_TRY(hipEventCreate(&set->sev[k]));
        set->sev_init = true;
    }
    hipEvent_t *ev = set->sev;
    int ng = int(set->ngroups);
    const DevPage *ts_pages = set->slots[0].dev[PC_RLE_TS];
    int nch_max = 0;
    for (int f = 0; f < nf; f++) {
        int nc = set->slots[1 + fields[f]].n_gor_chunks;
        nch_max = nc > nch_max ? nc : nch_max;
    }
    if (!set->d_gor_nactive &&
        hipMalloc(&set->d_gor_nactive, sizeof(int)) != hipSuccess)
        return fail(GS_ERR, "hipMalloc active counter failed");
    if (set->gor_active_cap < size_t(nch_max)) {
        if (set->d_gor_active) hipFree(set->d_gor_active);
        if (hipMalloc(&set->d_gor_active, size_t(nch_max) * sizeof(int)) !=
            hipSuccess)
            return fail(GS_ERR, "hipMalloc active list failed");
        set->gor_active_cap = size_t(nch_max);
    }
    int nblocks = (ng + SCAN_BLOCK * SCAN_ITEMS - 1) /
                  (SCAN_BLOCK * SCAN_ITEMS);
    if (nblocks > 2048)
        return fail(GS_ERR, "too many groups for the fused span scan");
    HIP_TRY(hipEventRecord(ev[SEV_START], ctx->stream));
    hipLaunchKernelGGL(k_spans_rle, dim3(grid_for(ng, 256)), dim3(256), 0,
                       ctx->stream, set->d_blob, ts_pages, ng,
                       spec->range.min_ts, spec->range.max_ts,
                       set->d_sp_start, set->d_sp_cnt, set->d_g_t0sel,
                       set->d_g_delta, ctx->d_err);
    /* device exclusive scan of span counts -> output offsets (+total) */
    hipLaunchKernelGGL(k_scan_partials, dim3(nblocks), dim3(SCAN_BLOCK), 0,
                       ctx->stream, set->d_sp_cnt, ng, set->d_out_off,
                       set->d_blocksums);
    hipLaunchKernelGGL(k_scan_fixup, dim3(1), dim3(64), 0, ctx->stream, ng,
                       set->d_out_off, set->d_blocksums, nblocks);
    hipLaunchKernelGGL(k_scan_add, dim3(grid_for(ng, 256)), dim3(256), 0,
                       ctx->stream, ng, set->d_out_off, set->d_blocksums);
    HIP_TRY(hipEventRecord(ev[SEV_OFFS], ctx->stream));
    /* at most every row of the set is selected: grid-stride beyond 2048
       blocks, and blocks past the device-side total exit at once */
    hipLaunchKernelGGL(k_rle_ts_tiles,
                       dim3(grid_for(set->total_rows, GS_TS_TILE)),
                       dim3(256), 0, ctx->stream, set->d_out_off, ng, set->d_g_t0sel,
                       set->d_g_delta, GS_TS_TILE, spec->d_out_ts);
    HIP_TRY(hipEventRecord(ev[SEV_TS], ctx->stream));
    int nsg = set->nsgroups;
    if (spec->n_buckets > 0) {
        if (!spec->d_agg_max || !spec->d_agg_sum || !spec->d_agg_count)
            return fail(GS_ERR, "agg outputs missing");
        size_t cells = size_t(nsg) * size_t(spec->n_buckets);
        if (set->partials_cap < cells) {
            if (set->d_pmax) hipFree(set->d_pmax);
            if (set->d_psum) hipFree(set->d_psum);
            if (set->d_pcnt) hipFree(set->d_pcnt);
            if (hipMalloc(&set->d_pmax, cells * 8) != hipSuccess ||
                hipMalloc(&set->d_psum, cells * 8) != hipSuccess ||
                hipMalloc(&set->d_pcnt, cells * 8) != hipSuccess)
                return fail(GS_ERR, "hipMalloc agg partials failed");
            set->partials_cap = cells;
        }
    }
    /* d_sgroups_out is read by the separate aggregate kernels only: built
       when the first field takes one of those branches, never on the
       fused path */
    bool sgroups_built = false;
    auto build_sgroups = [&]() {
        if (sgroups_built) return;
        hipLaunchKernelGGL(k_build_sgroups_out, dim3(grid_for(nsg, 256)),
                           dim3(256), 0, ctx->stream, set->d_sgroup_first,
                           nsg, set->d_out_off, set->d_sgroups_out);
        sgroups_built = true;
    };
    for (int f = 0; f < nf; f++) {
        SlotPages &fsp = set->slots[1 + fields[f]];
        int nch = fsp.n_gor_chunks;
        double *d_val_f = spec->d_out_val + size_t(f) * set->total_rows;
        HIP_TRY(hipMemsetAsync(set->d_gor_nactive, 0, sizeof(int),
                               ctx->stream));
        /* closed-form bucket boundaries via the RLE group table when it
           fits in LDS (it always does for realistic pages-per-series) */
        const size_t shm_rle =
            size_t(set->max_span) * 16 +
            (size_t(set->max_span) + size_t(spec->n_buckets) + 2) * 4;
        const bool rle_fits =
            spec->n_buckets <= 8192 && shm_rle <= 64 * 1024;
        /* Fused aggregate: the decode kernel accumulates the buckets and
           k_agg_fixup joins the pieces, in place of k_agg_partial_rle's
           second pass over the decoded values.  Each bucket boundary
           costs the decoding wave a divergent branch with three stores,
           so a bucket must span enough rows to pay for it. */
        const size_t shm_fix =
            (size_t(fsp.max_sg_chunks) * 2 * 4 + size_t(spec->n_buckets) +
             15) & ~size_t(15);
        bool agg_fused = false;
        if (spec->n_buckets > 0 && rle_fits && fsp.agg_fused_ok &&
            spec->bucket_ns > 0 && shm_fix <= 64 * 1024) {
            static int fused_env = [] { /* GS_AGG_FUSED=0: separate pass */
                const char *e = getenv("GS_AGG_FUSED");
                return e ? atoi(e) : 1;
            }();
            static long min_rows = [] { /* sweepable */
                const char *e = getenv("GS_AGG_FUSED_MIN_ROWS");
                long v = e ? atol(e) : 0;
                return v > 0 ? v : long(GS_AGG_FUSED_MIN_ROWS);
            }();
            agg_fused = fused_env != 0 &&
                        (set->min_pos_delta == INT64_MAX ||
                         spec->bucket_ns / set->min_pos_delta >= min_rows);
        }
        if (agg_fused && set->agg_pieces_cap < size_t(nch_max) * 2) {
            if (set->d_agg_meta) hipFree(set->d_agg_meta);
            if (set->d_agg_val) hipFree(set->d_agg_val);
            set->d_agg_meta = nullptr;
            set->d_agg_val = nullptr;
            set->agg_pieces_cap = 0;
            if (hipMalloc(&set->d_agg_meta, size_t(nch_max) * 2 *
                                                sizeof(DevAggMeta)) !=
                    hipSuccess ||
                hipMalloc(&set->d_agg_val, size_t(nch_max) * 2 *
                                               sizeof(DevAggVal)) !=
                    hipSuccess)
                return fail(GS_ERR, "hipMalloc agg pieces failed");
            set->agg_pieces_cap = size_t(nch_max) * 2;
        }
        hipLaunchKernelGGL(k_gor_active, dim3(grid_for(nch, 256)), dim3(256),
                           0, ctx->stream, fsp.d_gor_chunks, nch,
                           set->d_sp_start, set->d_sp_cnt, set->d_gor_active,
                           set->d_gor_nactive,
                           agg_fused ? set->d_agg_meta : nullptr);
        GorAggArgs ag{};
        if (agg_fused) {
            ag.grp_sg = set->d_grp_sgroup;
            ag.g_t0sel = set->d_g_t0sel;
            ag.g_delta = set->d_g_delta;
            ag.t0 = spec->t0;
            ag.bucket_ns = spec->bucket_ns;
            ag.nbuckets = spec->n_buckets;
            ag.pmax = set->d_pmax;
            ag.psum = set->d_psum;
            ag.pcnt = set->d_pcnt;
            ag.pc_meta = set->d_agg_meta;
            ag.pc_val = set->d_agg_val;
            hipLaunchKernelGGL(k_gor_chunks_filtered<true>,
                               dim3(grid_for(nch, GS_GOR_BLOCK)),
                               dim3(GS_GOR_BLOCK), 0, ctx->stream,
                               set->d_blob, fsp.d_gor_chunks,
                               set->d_gor_active, set->d_gor_nactive,
                               set->d_sp_start, set->d_sp_cnt,
                               set->d_out_off, d_val_f, ctx->d_err, ag);
        } else {
            hipLaunchKernelGGL(k_gor_chunks_filtered<false>,
                               dim3(grid_for(nch, GS_GOR_BLOCK)),
                               dim3(GS_GOR_BLOCK), 0, ctx->stream,
                               set->d_blob, fsp.d_gor_chunks,
                               set->d_gor_active, set->d_gor_nactive,
                               set->d_sp_start, set->d_sp_cnt,
                               set->d_out_off, d_val_f, ctx->d_err, ag);
        }
        if (f == 0) HIP_TRY(hipEventRecord(ev[SEV_VAL], ctx->stream));
        if (spec->n_buckets > 0) {
            if (agg_fused) {
                hipLaunchKernelGGL(k_agg_fixup,
                                   dim3(grid_items(nsg, 65535)),
                                   dim3(256), shm_fix, ctx->stream,
                                   set->d_agg_meta, set->d_agg_val,
                                   fsp.d_sg_chunk_first,
                                   nsg, spec->n_buckets,
                                   fsp.max_sg_chunks * 2, set->d_pmax,
                                   set->d_psum, set->d_pcnt);
            } else if (rle_fits) {
                static int agg_block = [] { /* sweepable (GS_AGG_BLOCK) */
                    const char *e = getenv("GS_AGG_BLOCK");
                    long v = e ? atol(e) : 0;
                    return int(v == 128 || v == 512 ? v : 256);
                }();
                build_sgroups();
                hipLaunchKernelGGL(k_agg_partial_rle,
                                   dim3(grid_items(nsg, 65535)),
                                   dim3(agg_block), shm_rle, ctx->stream,
                                   set->d_sgroups_out, nsg,
                                   set->d_sgroup_first, set->d_g_t0sel,
                                   set->d_g_delta, set->d_out_off, d_val_f,
                                   spec->t0, spec->bucket_ns,
                                   spec->n_buckets, set->max_span,
                                   set->d_pmax, set->d_psum, set->d_pcnt);
            } else {
                size_t agg_shm = spec->n_buckets <= 8192
                                     ? (size_t(spec->n_buckets) + 1) * 4
                                     : 0;
                build_sgroups();
                hipLaunchKernelGGL(
                    k_agg_partial, dim3(grid_items(nsg, 65535)),
                    dim3(256), agg_shm, ctx->stream, set->d_sgroups_out,
                    nsg, spec->d_out_ts, d_val_f, nullptr, INT64_MIN,
                    INT64_MAX, spec->t0, spec->bucket_ns, spec->n_buckets,
                    set->d_pmax, set->d_psum, set->d_pcnt);
            }
            int mb = (spec->n_buckets + 3) / 4;
            hipLaunchKernelGGL(k_agg_merge, dim3(grid_items(mb, 2048)),
                               dim3(256), 0, ctx->stream, nsg,
                               spec->n_buckets, set->d_pmax, set->d_psum,
                               set->d_pcnt,
                               spec->d_agg_max + size_t(f) * spec->n_buckets,
                               spec->d_agg_sum + size_t(f) * spec->n_buckets,
                               spec->d_agg_count +
                                   size_t(f) * spec->n_buckets);
        }
    }
    HIP_TRY(hipEventRecord(ev[SEV_END], ctx->stream));
    set->pending = true;
    return GS_OK;
}

/* Phase times from the events of scan_fused_launch: filter = spans +
 * offset scan, decode_ts = k_rle_ts_tiles, decode_val = k_gor_active +
 * the Gorilla decode of field 0, agg = everything after it.  With the
 * fused aggregate (GS_AGG_FUSED, the default where the gate passes)
 * decode_val includes the in-kernel bucket accumulation and agg covers
 * only k_agg_fixup + k_agg_merge; on the separate path agg is
 * k_agg_partial_rle (or k_agg_partial) + k_agg_merge as before. */
static GsStatus scan_fused_wait(GsCtx *ctx, GsGroupSet *set,
                                GsScanResult *result) {
    if (!set->pending)
        return fail(GS_ERR, "no fused scan in flight on this set");
    set->pending = false;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    GsStatus st = check_dev_err(ctx);
    if (st != GS_OK) return st;
    int64_t acc = 0;
    HIP_TRY(hipMemcpy(&acc, set->d_out_off + set->ngroups, sizeof(int64_t),
                      hipMemcpyDeviceToHost));
    hipEvent_t *ev = set->sev;
    float ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[SEV_START], ev[SEV_OFFS]));
    result->ms_filter = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[SEV_OFFS], ev[SEV_TS]));
    result->ms_decode_ts = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[SEV_TS], ev[SEV_VAL]));
    result->ms_decode_val = ms; /* nf>1: field 0 only */
    result->ms_compact = 0.0;
    HIP_TRY(hipEventElapsedTime(&ms, ev[SEV_VAL], ev[SEV_END]));
    result->ms_agg = ms; /* fused aggregate: fix-up + merge only.
                            nf>1: field 0's agg + remaining fields */
    result->out_rows = acc;
    result->decoded_rows = set->total_rows;
    return GS_OK;
}

GsStatus gs_scan_async(GsCtx *ctx, GsGroupSet *set, const GsScanSpec *spec) {
    if (!ctx || !set || !spec)
        return fail(GS_ERR, "bad args to gs_scan_async");
    if (!fused_capable(set, spec))
        return fail(GS_ERR, "gs_scan_async requires the fused-capable shape "
                            "(RLE ts + all-valid Gorilla, no tombstones, "
                            "compacted outputs)");
    int32_t f0 = spec->field_col;
    return scan_fused_launch(ctx, set, spec, &f0, 1);
}

GsStatus gs_scan_wait(GsCtx *ctx, GsGroupSet *set, GsScanResult *result) {
    if (!ctx || !set || !result)
        return fail(GS_ERR, "bad args to gs_scan_wait");
    return scan_fused_wait(ctx, set, result);
}

/* Raw row set: series structure over caller-resident DEVICE arrays with
 * no pages — the memcache leg (MemCacheReader rows,
 * mem_cache/series_data.rs:15-27).  gs_scan over such a set skips the
 * decode phases and filters/aggregates spec->d_ts / spec->d_val
 * directly; rows are taken as non-null (pre-filter nulls when building
 * the arrays).  counts[i] = rows of series i (time-sorted). */
GsGroupSet *gs_raw_set(GsCtx *ctx, const int64_t *counts, int64_t nseries) {
    if (!ctx || !counts || nseries <= 0) {
        fail(GS_ERR, "bad args to gs_raw_set");
        return nullptr;
    }
    if (hipSetDevice(ctx->device) != hipSuccess) {
        fail(GS_ERR, "hipSetDevice failed");
        return nullptr;
    }
    GsGroupSet *set = new GsGroupSet();
    set->ctx = ctx;
    set->ngroups = size_t(nseries);
    set->ncols = 0;
    set->row_offsets.resize(nseries);
    std::vector<DevGroup> hg(nseries);
    int64_t rows = 0;
    for (int64_t i = 0; i < nseries; i++) {
        if (counts[i] < 0 || counts[i] > INT32_MAX) {
            fail(GS_ERR, "raw set series row count out of range");
            gs_groups_free(set);
            return nullptr;
        }
        set->row_offsets[i] = rows;
        hg[i].row_off = rows;
        hg[i].nrows = int32_t(counts[i]);
        hg[i].pad = 0;
        rows += counts[i];
    }
    set->total_rows = rows;
    set->nsgroups = int(nseries);
    set->sgroup_span.assign(nseries, 1);
    set->max_span = 1;
    std::vector<int32_t> sgfirst(nseries + 1);
    for (int64_t i = 0; i <= nseries; i++) sgfirst[i] = int32_t(i);
    size_t nblocks = (size_t(nseries) + SCAN_BLOCK * SCAN_ITEMS - 1) /
                     (SCAN_BLOCK * SCAN_ITEMS);
    if (hipMalloc(&set->d_groups, nseries * sizeof(DevGroup)) != hipSuccess ||
        hipMalloc(&set->d_sgroups, nseries * sizeof(DevGroup)) != hipSuccess ||
        hipMalloc(&set->d_sgroups_out, nseries * sizeof(DevGroup)) != hipSuccess ||
        hipMalloc(&set->d_sgroup_first, sgfirst.size() * sizeof(int32_t)) != hipSuccess ||
        hipMalloc(&set->d_sp_start, nseries * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_sp_cnt, nseries * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_out_off, (nseries + 1) * sizeof(int64_t)) != hipSuccess ||
        hipMalloc(&set->d_blocksums, (nblocks + 1) * sizeof(int64_t)) != hipSuccess) {
        fail(GS_ERR, "hipMalloc raw set tables failed");
        gs_groups_free(set);
        return nullptr;
    }
    hipMemcpyAsync(set->d_groups, hg.data(), nseries * sizeof(DevGroup),
                   hipMemcpyHostToDevice, ctx->stream);
    hipMemcpyAsync(set->d_sgroups, hg.data(), nseries * sizeof(DevGroup),
                   hipMemcpyHostToDevice, ctx->stream);
    hipMemcpyAsync(set->d_sgroup_first, sgfirst.data(),
                   sgfirst.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                   ctx->stream);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) {
        fail(GS_ERR, "raw set upload failed");
        gs_groups_free(set);
        return nullptr;
    }
    return set;
}

/* Fused scan of nf field columns over ONE span/ts pass (TSBS
 * cpu-max-all-8, BASELINE config #3; the reference decodes each field
 * column of the column group in the same decode_pages pass,
 * tsm/reader.rs:494-560).  Fused-capable shapes only.  Strides:
 * d_out_val + f*total_rows per field; d_agg_* + f*n_buckets per field. */
GsStatus gs_scan_fields(GsCtx *ctx, GsGroupSet *set, const GsScanSpec *spec,
                        const int32_t *field_cols, int nf,
                        GsScanResult *result) {
    if (!ctx || !set || !spec || !result || !field_cols || nf <= 0)
        return fail(GS_ERR, "bad args to gs_scan_fields");
    if (!fused_capable_fields(set, spec, field_cols, nf))
        return fail(GS_ERR, "gs_scan_fields needs a fused-capable shape "
                            "(all-RLE ts, all-valid Gorilla fields, no "
                            "tombstones/predicates, compacted outputs)");
    GsStatus st = scan_fused_launch(ctx, set, spec, field_cols, nf);
    if (st != GS_OK) return st;
    return scan_fused_wait(ctx, set, result);
}

/* async variant: pair with gs_scan_wait */
GsStatus gs_scan_fields_async(GsCtx *ctx, GsGroupSet *set,
                              const GsScanSpec *spec,
                              const int32_t *field_cols, int nf) {
    if (!ctx || !set || !spec || !field_cols || nf <= 0)
        return fail(GS_ERR, "bad args to gs_scan_fields_async");
    if (!fused_capable_fields(set, spec, field_cols, nf))
        return fail(GS_ERR, "gs_scan_fields needs a fused-capable shape");
    return scan_fused_launch(ctx, set, spec, field_cols, nf);
}

GsStatus gs_scan(GsCtx *ctx, GsGroupSet *set, const GsScanSpec *spec,
                 GsScanResult *result) {
    if (!ctx || !set || !spec || !result || !spec->d_ts || !spec->d_val)
        return fail(GS_ERR, "bad args to gs_scan");
    const bool raw = set->ncols == 0; /* gs_raw_set: memcache rows already
                                         resident in spec->d_ts/d_val */
    if (!raw) {
        if (set->ncols < 2)
            return fail(GS_ERR, "gs_scan needs a time page + one f64 field page");
        const uint32_t fcol = 1 + uint32_t(spec->field_col);
        if (spec->field_col < 0 || fcol >= set->ncols)
            return fail(GS_ERR, "gs_scan field column out of range");
        const uint8_t fct2 = set->slots[fcol].ctype;
        if (fct2 != GS_CT_F64 && fct2 != GS_CT_I64 && fct2 != GS_CT_U64)
            return fail(GS_ERR,
                        "gs_scan field column must be f64/i64/u64");
        if (fct2 != GS_CT_F64 && spec->n_buckets > 0)
            return fail(GS_ERR, "aggregates are f64-only (TSBS path); "
                                "decode+filter+compact support i64/u64");
    }
    HIP_TRY(hipSetDevice(ctx->device));

    /* per-phase timing on the engine stream (HIP events) */
    hipEvent_t ev[6];
    for (int k = 0; k < 6; k++) HIP_TRY(hipEventCreate(&ev[k]));
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard() { for (int k = 0; k < 6; k++) hipEventDestroy(e[k]); }
    } guard{ev};

    /* fused filtered path: spans closed-form from RLE ts headers, Gorilla
     * decode writes only the selected rows already compacted, aggregate
     * runs over the compacted output.  Preconditions: every ts page RLE,
     * every field page all-valid Gorilla, no tombstones, compacted
     * outputs requested.  Falls back to the general path otherwise. */
    if (fused_capable(set, spec)) {
        int32_t f0 = spec->field_col;
        GsStatus fst = scan_fused_launch(ctx, set, spec, &f0, 1);
        if (fst != GS_OK) return fst;
        return scan_fused_wait(ctx, set, result);
    }

    /* validity bytes needed if the field has nulls or tombstones apply */
    uint8_t *d_valid = nullptr;
    bool need_valid = set->any_nulls_field || spec->n_tombstones > 0;
    if (need_valid) {
        if (!set->d_valid)
            HIP_TRY(hipMalloc(&set->d_valid, size_t(set->total_rows)));
        d_valid = set->d_valid;
    }

    HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    GsStatus st;
    if (!raw) {
        st = gs_decode(ctx, set, 0, spec->d_ts, nullptr);
        if (st != GS_OK) return st;
    }
    HIP_TRY(hipEventRecord(ev[1], ctx->stream));
    if (!raw) {
        st = gs_decode(ctx, set, 1 + uint32_t(spec->field_col), spec->d_val,
                       d_valid);
        if (st != GS_OK) return st;
    } else if (d_valid) {
        /* raw rows are non-null; tombstones clear from an all-valid base */
        HIP_TRY(hipMemsetAsync(d_valid, 1, size_t(set->total_rows),
                               ctx->stream));
    }
    HIP_TRY(hipEventRecord(ev[2], ctx->stream));

    if (spec->n_tombstones > 0) {
        st = gs_apply_tombstone(ctx, set, spec->d_ts, d_valid,
                                spec->tombstones, spec->n_tombstones);
        if (st != GS_OK) return st;
    }

    int ng = int(set->ngroups);
    hipLaunchKernelGGL(k_spans, dim3(grid_for(ng, 256)), dim3(256), 0,
                       ctx->stream, set->d_groups, ng, spec->d_ts,
                       spec->range.min_ts, spec->range.max_ts, set->d_sp_start,
                       set->d_sp_cnt);

    /* optional value predicate (DataFilter, reader/filter.rs:91-142) */
    uint8_t *d_mask = nullptr;
    const int64_t *d_counts = set->d_sp_cnt;
    if (spec->value_pred.op != GS_PRED_NONE) {
        if (!set->d_mask)
            HIP_TRY(hipMalloc(&set->d_mask, size_t(set->total_rows)));
        if (!set->d_sel_cnt)
            HIP_TRY(hipMalloc(&set->d_sel_cnt,
                              set->ngroups * sizeof(int64_t)));
        d_mask = set->d_mask;
        int vt = 0; /* raw (memcache) sets have no column slots: f64 */
        if (!raw) {
            const uint8_t fct = set->slots[1 + spec->field_col].ctype;
            vt = fct == GS_CT_I64 ? 1 : fct == GS_CT_U64 ? 2 : 0;
        }
        hipLaunchKernelGGL(k_vmask, dim3(grid_items(ng, 65535)), dim3(256),
                           0, ctx->stream, set->d_groups, ng, spec->d_val,
                           d_valid, set->d_sp_start, set->d_sp_cnt,
                           spec->value_pred.op, spec->value_pred.a,
                           spec->value_pred.b, vt, d_mask, set->d_sel_cnt);
        d_counts = set->d_sel_cnt;
    }
    HIP_TRY(hipEventRecord(ev[3], ctx->stream));

    bool want_rows = spec->d_out_ts && spec->d_out_val;
    {
        /* device exclusive scan of selected counts -> offsets + total:
           no host round-trip mid-pipeline (the round-1 version
           synchronized here and prefix-summed on the host) */
        int nblocks = (ng + SCAN_BLOCK * SCAN_ITEMS - 1) /
                      (SCAN_BLOCK * SCAN_ITEMS);
        if (nblocks > 2048)
            return fail(GS_ERR, "too many groups for the span scan");
        hipLaunchKernelGGL(k_scan_partials, dim3(nblocks), dim3(SCAN_BLOCK),
                           0, ctx->stream, d_counts, ng, set->d_out_off,
                           set->d_blocksums);
        hipLaunchKernelGGL(k_scan_fixup, dim3(1), dim3(64), 0, ctx->stream,
                           ng, set->d_out_off, set->d_blocksums, nblocks);
        hipLaunchKernelGGL(k_scan_add, dim3(grid_for(ng, 256)), dim3(256), 0,
                           ctx->stream, ng, set->d_out_off, set->d_blocksums);
        if (want_rows) {
            if (d_mask)
                hipLaunchKernelGGL(k_compact_masked,
                                   dim3(grid_items(ng, 2048)), dim3(256), 0,
                                   ctx->stream, set->d_groups, ng, spec->d_ts,
                                   spec->d_val, d_mask, set->d_sp_start,
                                   set->d_sp_cnt, set->d_out_off,
                                   spec->d_out_ts, spec->d_out_val);
            else
                hipLaunchKernelGGL(k_compact, dim3(grid_items(ng, 2048)),
                                   dim3(256), 0, ctx->stream, set->d_groups,
                                   ng, spec->d_ts, spec->d_val,
                                   set->d_sp_start, set->d_sp_cnt,
                                   set->d_out_off, spec->d_out_ts,
                                   spec->d_out_val);
        }
    }
    HIP_TRY(hipEventRecord(ev[4], ctx->stream));

    if (spec->n_buckets > 0) {
        if (!spec->d_agg_max || !spec->d_agg_sum || !spec->d_agg_count)
            return fail(GS_ERR, "agg outputs missing");
        int nsg = set->nsgroups;
        size_t cells = size_t(nsg) * size_t(spec->n_buckets);
        if (set->partials_cap < cells) {
            if (set->d_pmax) hipFree(set->d_pmax);
            if (set->d_psum) hipFree(set->d_psum);
            if (set->d_pcnt) hipFree(set->d_pcnt);
            if (hipMalloc(&set->d_pmax, cells * 8) != hipSuccess ||
                hipMalloc(&set->d_psum, cells * 8) != hipSuccess ||
                hipMalloc(&set->d_pcnt, cells * 8) != hipSuccess)
                return fail(GS_ERR, "hipMalloc agg partials failed");
            set->partials_cap = cells;
        }
        size_t agg_shm = spec->n_buckets <= 8192
                             ? (size_t(spec->n_buckets) + 1) * 4 : 0;
        hipLaunchKernelGGL(k_agg_partial, dim3(grid_items(nsg, 65535)),
                           dim3(256), agg_shm, ctx->stream, set->d_sgroups, nsg,
                           spec->d_ts, spec->d_val,
                           d_mask ? d_mask : d_valid,
                           spec->range.min_ts, spec->range.max_ts,
                           spec->t0, spec->bucket_ns,
                           spec->n_buckets, set->d_pmax, set->d_psum,
                           set->d_pcnt);
        int mb = (spec->n_buckets + 3) / 4;
        hipLaunchKernelGGL(k_agg_merge, dim3(grid_items(mb, 2048)), dim3(256),
                           0, ctx->stream, nsg, spec->n_buckets, set->d_pmax,
                           set->d_psum, set->d_pcnt, spec->d_agg_max,
                           spec->d_agg_sum, spec->d_agg_count);
    }
    HIP_TRY(hipEventRecord(ev[5], ctx->stream));

    HIP_TRY(hipStreamSynchronize(ctx->stream));
    st = check_dev_err(ctx);
    if (st != GS_OK) return st;
    float ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    result->ms_decode_ts = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[1], ev[2]));
    result->ms_decode_val = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[2], ev[3]));
    result->ms_filter = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[3], ev[4]));
    result->ms_compact = ms;
    HIP_TRY(hipEventElapsedTime(&ms, ev[4], ev[5]));
    result->ms_agg = ms;

    int64_t out_rows = 0;
    HIP_TRY(hipMemcpy(&out_rows, set->d_out_off + set->ngroups,
                      sizeof(int64_t), hipMemcpyDeviceToHost));
    result->out_rows = out_rows;
    result->decoded_rows = set->total_rows;
    return GS_OK;
}

/* Worst-case data block of an 8-byte column page of maxr rows, as the
 * device entry points ask for it (ints: 16 bytes above the host's
 * threshold, see tsm_int_max_len). */
static int64_t enc_dev_max_len(bool f64, int64_t maxr) {
    return f64 ? int64_t(tsm_gorilla_max_len(uint64_t(maxr)))
               : int64_t(tsm_int_max_len(uint64_t(maxr))) + 16;
}

/* After an encode launch: the encoders' own error surface.  Pages (cells)
 * that failed have a negative length, every other one of the launch is
 * complete. */
static GsStatus enc_dev_status(GsCtx *ctx, const char *null_row_msg) {
    unsigned e = 0;
    HIP_TRY(hipMemcpy(&e, ctx->d_err, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (!e) return GS_OK;
    hipMemset(ctx->d_err, 0, sizeof(unsigned));
    if (e & DERR_ENC_SENTINEL)
        return fail(GS_ERR_SENTINEL,
                    "encode: Gorilla sentinel value in the input");
    if (e & DERR_ENC_NULL) return fail(GS_ERR_FORMAT, null_row_msg);
    return fail(GS_ERR_FORMAT, "encode: value out of simple8b range");
}

/* Both encode entries.  no_nulls: every column refuses a page with a null
 * row, as the time column always does; null_row_msg is that refusal's
 * message. */
static GsStatus enc_group_pages(GsCtx *ctx, int32_t ncols,
                                const uint8_t *ctype,
                                const void *const *d_vals,
                                const uint8_t *const *d_valid,
                                const int64_t *h_row_off,
                                const int32_t *h_rows, int32_t npages,
                                uint8_t *const *d_out,
                                const int64_t *cap_per_page,
                                GsPageInfo *h_info, bool no_nulls,
                                const char *null_row_msg) {
    if (ncols < 1 || ncols > GS_MAX_ENCODE_COLS)
        return fail(GS_ERR, "gs_encode_group_pages_dev: ncols outside "
                            "1..GS_MAX_ENCODE_COLS");
    if (!ctx || !ctype || !d_vals || !h_row_off || !h_rows || !d_out ||
        !cap_per_page || !h_info)
        return fail(GS_ERR, "gs_encode_group_pages_dev: NULL argument");
    if (npages <= 0)
        return fail(GS_ERR, "gs_encode_group_pages_dev: npages <= 0");
    if (int64_t(ncols) * npages > INT32_MAX)
        return fail(GS_ERR, "gs_encode_group_pages_dev: too many pages");
    int64_t maxr = 0, extent = 0;
    for (int32_t p = 0; p < npages; p++) {
        if (h_rows[p] < 0 || h_row_off[p] < 0)
            return fail(GS_ERR, "gs_encode_group_pages_dev: negative page "
                                "offset or row count");
        if (h_rows[p] > maxr) maxr = h_rows[p];
        if (h_row_off[p] + h_rows[p] > extent) extent = h_row_off[p] + h_rows[p];
    }
    for (int32_t c = 0; c < ncols; c++) {
        if (ctype[c] != GS_CT_TIME && ctype[c] != GS_CT_I64 &&
            ctype[c] != GS_CT_F64 && ctype[c] != GS_CT_BOOL &&
            ctype[c] != GS_CT_U64)
            return fail(GS_ERR, "gs_encode_group_pages_dev: column type must "
                                "be time, i64, f64, bool or u64 (strings use "
                                "gs_encode_str)");
        if (!d_vals[c] || !d_out[c])
            return fail(GS_ERR, "gs_encode_group_pages_dev: NULL column "
                                "buffer");
    }
    for (int32_t c = 0; c < ncols; c++) {
        /* worst case: ints -> uncompressed 8 B/val; f64 -> ~77 bits/val;
           bool -> header, 10-byte varint bound and one bit per value */
        int64_t need = 16 + (maxr + 7) / 8;
        if (ctype[c] == GS_CT_BOOL) need += 2 + 10 + (maxr + 7) / 8;
        else need += enc_dev_max_len(ctype[c] == GS_CT_F64, maxr);
        if (cap_per_page[c] < need)
            return fail(GS_ERR_CAP, "gs_encode_group_pages_dev: cap_per_page "
                                    "below worst-case encoded size");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t nwork = size_t(ncols) * size_t(npages);
    std::vector<void *> scratch;
    auto release = [&]() { for (void *q : scratch) hipFree(q); };
    auto dalloc = [&](size_t bytes) -> void * {
        void *q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess) return nullptr;
        scratch.push_back(q);
        return q;
    };
    std::vector<EncGroupCol> cols(ncols);
    for (int32_t c = 0; c < ncols; c++) {
        cols[c].vals = d_vals[c];
        cols[c].valid = d_valid ? d_valid[c] : nullptr;
        cols[c].dense = nullptr;
        cols[c].out = d_out[c];
        cols[c].cap = cap_per_page[c];
        cols[c].ctype = ctype[c];
        cols[c].flags = no_nulls ? ENC_COL_NO_NULLS : 0;
        if (cols[c].valid) { /* only null-carrying columns are densified */
            cols[c].dense =
                dalloc(size_t(extent) * (ctype[c] == GS_CT_BOOL ? 1 : 8));
            if (!cols[c].dense) {
                release();
                return fail(GS_ERR, "hipMalloc dense scratch failed");
            }
        }
    }
    std::vector<EncPageSpec> specs(npages);
    for (int32_t p = 0; p < npages; p++) {
        specs[p].row_off = h_row_off[p];
        specs[p].nrows = h_rows[p];
        specs[p].pad = 0;
    }
    EncGroupCol *d_cols = (EncGroupCol *)dalloc(cols.size() * sizeof(EncGroupCol));
    EncPageSpec *d_specs = (EncPageSpec *)dalloc(specs.size() * sizeof(EncPageSpec));
    int32_t *d_cnt = (int32_t *)dalloc(nwork * sizeof(int32_t));
    GsPageInfo *d_info = (GsPageInfo *)dalloc(nwork * sizeof(GsPageInfo));
    if (!d_cols || !d_specs || !d_cnt || !d_info) {
        release();
        return fail(GS_ERR, "hipMalloc encode tables failed");
    }
    hipMemcpyAsync(d_cols, cols.data(), cols.size() * sizeof(EncGroupCol),
                   hipMemcpyHostToDevice, ctx->stream);
    hipMemcpyAsync(d_specs, specs.data(), specs.size() * sizeof(EncPageSpec),
                   hipMemcpyHostToDevice, ctx->stream);
    hipLaunchKernelGGL(k_enc_prepare, dim3(grid_for(int(nwork), 1)),
                       dim3(ENC_PREP_THREADS), 0, ctx->stream, d_cols, ncols,
                       d_specs, npages, d_cnt, d_info);
    /* thread per page: 64-thread blocks spread the serial encoders over
       more CUs than 256-thread blocks would */
    hipLaunchKernelGGL(k_enc_group_pages, dim3(grid_for(int(nwork), 64)),
                       dim3(64), 0, ctx->stream, d_cols, ncols, d_specs,
                       npages, d_cnt, d_info, ctx->d_err);
    GsStatus st = GS_OK;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess)
        st = fail(GS_ERR, "group encode kernels failed");
    else if (hipMemcpy(h_info, d_info, nwork * sizeof(GsPageInfo),
                       hipMemcpyDeviceToHost) != hipSuccess)
        st = fail(GS_ERR, "group encode: page info readback failed");
    release();
    if (st != GS_OK) return st;
    return enc_dev_status(ctx, null_row_msg);
}

GsStatus gs_encode_group_pages_dev(GsCtx *ctx, int32_t ncols,
                                   const uint8_t *ctype,
                                   const void *const *d_vals,
                                   const uint8_t *const *d_valid,
                                   const int64_t *h_row_off,
                                   const int32_t *h_rows, int32_t npages,
                                   uint8_t *const *d_out,
                                   const int64_t *cap_per_page,
                                   GsPageInfo *h_info) {
    return enc_group_pages(ctx, ncols, ctype, d_vals, d_valid, h_row_off,
                           h_rows, npages, d_out, cap_per_page, h_info, false,
                           "encode: null row in the time column");
}

/* one column of the group encode; the statistics are dropped */
GsStatus gs_encode_pages_dev(GsCtx *ctx, int32_t kind, const void *d_vals,
                             const uint8_t *d_valid, const int64_t *h_row_off,
                             const int32_t *h_rows, int32_t npages,
                             uint8_t *d_out, int64_t cap_per_page,
                             int64_t *h_lens) {
    if (!ctx || !d_vals || !h_row_off || !h_rows || npages <= 0 || !d_out ||
        !h_lens || kind < 0 || kind > 2)
        return fail(GS_ERR, "bad args to gs_encode_pages_dev");
    const uint8_t ctype =
        kind == 0 ? GS_CT_TIME : kind == 1 ? GS_CT_I64 : GS_CT_F64;
    std::vector<GsPageInfo> info(npages);
    GsStatus st = enc_group_pages(
        ctx, 1, &ctype, &d_vals, &d_valid, h_row_off, h_rows, npages, &d_out,
        &cap_per_page, info.data(), kind == 1,
        "encode: null row in a ts/i64 page (integer pages must be all-valid)");
    /* with these three the launch ran and every page has its length */
    if (st == GS_OK || st == GS_ERR_FORMAT || st == GS_ERR_SENTINEL)
        for (int32_t p = 0; p < npages; p++) h_lens[p] = info[p].len;
    return st;
}

/* String pages: measure, check and lay out on the host, encode. */
GsStatus gs_encode_str_pages_dev(GsCtx *ctx, const int64_t *d_offsets,
                                 const uint8_t *d_bytes,
                                 const uint8_t *d_valid,
                                 const int64_t *h_row_off,
                                 const int32_t *h_rows, int32_t npages,
                                 uint8_t *d_out, int64_t cap_per_page,
                                 GsPageInfo *h_info) {
    if (!ctx || !d_offsets || !d_bytes || !h_row_off || !h_rows || !d_out ||
        !h_info)
        return fail(GS_ERR, "gs_encode_str_pages_dev: NULL argument");
    if (npages <= 0)
        return fail(GS_ERR, "gs_encode_str_pages_dev: npages <= 0");
    for (int32_t p = 0; p < npages; p++)
        if (h_rows[p] < 0 || h_row_off[p] < 0)
            return fail(GS_ERR, "gs_encode_str_pages_dev: negative page "
                                "offset or row count");
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<void *> scratch;
    auto release = [&]() { for (void *q : scratch) hipFree(q); };
    auto dalloc = [&](size_t bytes) -> void * {
        void *q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess) return nullptr;
        scratch.push_back(q);
        return q;
    };
    std::vector<EncPageSpec> specs(npages);
    for (int32_t p = 0; p < npages; p++) {
        specs[p].row_off = h_row_off[p];
        specs[p].nrows = h_rows[p];
        specs[p].pad = 0;
    }
    EncPageSpec *d_specs = (EncPageSpec *)dalloc(specs.size() * sizeof(EncPageSpec));
    StrEncMeasure *d_meas =
        (StrEncMeasure *)dalloc(size_t(npages) * sizeof(StrEncMeasure));
    int64_t *d_slab_off = (int64_t *)dalloc(size_t(npages) * sizeof(int64_t));
    GsPageInfo *d_info = (GsPageInfo *)dalloc(size_t(npages) * sizeof(GsPageInfo));
    if (!d_specs || !d_meas || !d_slab_off || !d_info) {
        release();
        return fail(GS_ERR, "hipMalloc string encode tables failed");
    }
    hipMemcpyAsync(d_specs, specs.data(), specs.size() * sizeof(EncPageSpec),
                   hipMemcpyHostToDevice, ctx->stream);
    hipLaunchKernelGGL(k_str_enc_measure, dim3(grid_for(npages, 1)),
                       dim3(STR_ENC_THREADS), 0, ctx->stream, d_offsets,
                       d_valid, d_specs, npages, d_meas);
    std::vector<StrEncMeasure> meas(npages);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(meas.data(), d_meas, meas.size() * sizeof(StrEncMeasure),
                  hipMemcpyDeviceToHost) != hipSuccess) {
        release();
        return fail(GS_ERR, "string encode: measure pass failed");
    }
    std::vector<int64_t> slab_off(npages);
    int64_t slab_total = 0;
    for (int32_t p = 0; p < npages; p++) {
        if (meas[p].bad) {
            release();
            return fail(GS_ERR_FORMAT, "gs_encode_str_pages_dev: offsets "
                                       "decrease inside a page");
        }
        const int64_t need = 16 + (int64_t(h_rows[p]) + 7) / 8 +
                             int64_t(str_enc_max_len(uint64_t(meas[p].payload)));
        if (cap_per_page < need) {
            release();
            return fail(GS_ERR_CAP, "gs_encode_str_pages_dev: cap_per_page "
                                    "below worst-case encoded size");
        }
        slab_off[p] = slab_total;
        slab_total += meas[p].payload;
    }
    uint8_t *d_slabs = (uint8_t *)dalloc(size_t(slab_total));
    if (!d_slabs) {
        release();
        return fail(GS_ERR, "hipMalloc string payload slabs failed");
    }
    hipMemcpyAsync(d_slab_off, slab_off.data(), slab_off.size() * sizeof(int64_t),
                   hipMemcpyHostToDevice, ctx->stream);
    hipLaunchKernelGGL(k_str_enc_pages, dim3(grid_for(npages, 1)),
                       dim3(STR_ENC_THREADS), 0, ctx->stream, d_offsets, d_bytes,
                       d_valid, d_specs, npages, d_slab_off, d_slabs, d_out,
                       cap_per_page, d_info, ctx->d_err);
    GsStatus st = GS_OK;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess)
        st = fail(GS_ERR, "string encode kernel failed");
    else if (hipMemcpy(h_info, d_info, size_t(npages) * sizeof(GsPageInfo),
                       hipMemcpyDeviceToHost) != hipSuccess)
        st = fail(GS_ERR, "string encode: page info readback failed");
    release();
    return st;
}

/* Host-side setup of the merge: everything that depends
 * on the timestamps only.  Allocates the per-stream flag/prefix scratch,
 * runs k_cm_flags + k_cm_prefix once, and turns the per-(stream, series)
 * owner counts into per-series output offsets (host copy in ooff, device
 * copy enqueued on the ctx stream).  The caller launches the scatter
 * kernel, synchronizes, and frees plan.scratch. */
namespace {
struct CmPlan {
    CompactArgs a;
    std::vector<void *> scratch;
    std::vector<int64_t> ooff; /* [nseries+1] */
    int nseries = 0;
    int gx = 0;
    void release() {
        for (void *p : scratch) hipFree(p);
        scratch.clear();
    }
};

GsStatus cm_plan_ranks(GsCtx *ctx, GsGroupSet *const *sets, int32_t nsets,
                       const int64_t *const *d_ts, CmPlan &pl) {
    const int nseries = pl.nseries;
    CompactArgs &a = pl.a;
    memset(&a, 0, sizeof(a));
    for (int f = 0; f < nsets; f++) {
        a.ts[f] = d_ts[f];
        a.groups[f] = sets[f]->d_sgroups;
        size_t rows = size_t(sets[f]->total_rows);
        uint8_t *fl;
        int32_t *pf;
        if (hipMalloc(&fl, rows ? rows : 1) != hipSuccess)
            return fail(GS_ERR, "hipMalloc compact scratch failed");
        pl.scratch.push_back(fl);
        if (hipMalloc(&pf, (rows ? rows : 1) * 4) != hipSuccess)
            return fail(GS_ERR, "hipMalloc compact scratch failed");
        pl.scratch.push_back(pf);
        a.flags[f] = fl;
        a.prefix[f] = pf;
    }
    int64_t *d_counts, *d_ooff;
    if (hipMalloc(&d_counts, size_t(nsets) * nseries * 8) != hipSuccess)
        return fail(GS_ERR, "hipMalloc compact tables failed");
    pl.scratch.push_back(d_counts);
    if (hipMalloc(&d_ooff, size_t(nseries) * 8) != hipSuccess)
        return fail(GS_ERR, "hipMalloc compact tables failed");
    pl.scratch.push_back(d_ooff);
    a.counts = d_counts;
    a.out_off = d_ooff;

    pl.gx = grid_items(nseries, 2048);
    hipLaunchKernelGGL(k_cm_flags, dim3(pl.gx, nsets), dim3(256), 0,
                       ctx->stream, a, nsets, nseries, ctx->d_err);
    int total = nsets * nseries;
    hipLaunchKernelGGL(k_cm_prefix,
                       dim3(grid_items(total, 65535)), dim3(256), 0,
                       ctx->stream, a, nsets, nseries);
    std::vector<int64_t> counts(size_t(nsets) * nseries);
    pl.ooff.assign(size_t(nseries) + 1, 0);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(counts.data(), d_counts, counts.size() * 8,
                      hipMemcpyDeviceToHost));
    int64_t acc = 0;
    for (int s = 0; s < nseries; s++) {
        pl.ooff[s] = acc;
        for (int f = 0; f < nsets; f++) acc += counts[size_t(f) * nseries + s];
    }
    pl.ooff[nseries] = acc;
    HIP_TRY(hipMemcpyAsync(d_ooff, pl.ooff.data(), size_t(nseries) * 8,
                           hipMemcpyHostToDevice, ctx->stream));
    return GS_OK;
}
} // namespace

namespace {
/* The merge behind gs_compact_merge, gs_compact_merge_fields (nstr == 0)
 * and gs_compact_merge_group: the timestamp rank work runs once for any mix
 * of columns.  `who` names the entry in messages. */
GsStatus cm_merge_group(GsCtx *ctx, GsGroupSet *const *sets, int32_t nsets,
                        int32_t ncols, const int32_t *elem_size,
                        const int64_t *const *d_ts, const void *const *d_val,
                        const uint8_t *const *d_valid, int32_t nstr,
                        const GsStrColumn *str_in, int64_t *d_out_ts,
                        void *const *d_out_val, uint8_t *const *d_out_valid,
                        GsStrColumnOut *str_out, int64_t *h_out_offsets,
                        int64_t *out_rows, const char *who) {
    auto bad = [&](GsStatus st, const char *msg) {
        return fail(st, (std::string(who) + ": " + msg).c_str());
    };
    if (!ctx || !sets || !d_ts || !d_out_ts ||
        (ncols > 0 && (!elem_size || !d_val || !d_out_val)) ||
        (nstr > 0 && (!str_in || !str_out)))
        return bad(GS_ERR, "NULL argument");
    if (nsets < 1 || nsets > GS_MAX_STREAMS)
        return bad(GS_ERR, "nsets outside 1..GS_MAX_STREAMS");
    const int nc = ncols + nstr;
    if (ncols < 0 || nstr < 0 || nc < 1 || nc > GS_MAX_MERGE_COLS)
        return bad(GS_ERR, "ncols + nstr outside 1..GS_MAX_MERGE_COLS");
    uint32_t wide = 0;
    for (int c = 0; c < ncols; c++) {
        if (elem_size[c] != 8 && elem_size[c] != 1)
            return bad(GS_ERR, "elem_size must be 8 or 1");
        if (!d_out_val[c]) return bad(GS_ERR, "NULL output column");
        if (elem_size[c] == 8) wide |= 1u << c;
    }
    for (int c = 0; c < nstr; c++) {
        if (!str_out[c].d_offsets || !str_out[c].d_bytes ||
            str_out[c].bytes_cap < 0)
            return bad(GS_ERR, "NULL string output column");
        wide |= 1u << (ncols + c);
    }
    for (int f = 0; f < nsets; f++)
        if (!sets[f] || !d_ts[f]) return bad(GS_ERR, "NULL stream");
    for (int i = 0; i < nsets * nstr; i++)
        if (str_in[i].d_offsets && !str_in[i].d_bytes)
            return bad(GS_ERR, "string column without bytes");
    int nseries = sets[0]->nsgroups;
    for (int f = 0; f < nsets; f++)
        if (sets[f]->nsgroups != nseries)
            return fail(GS_ERR, "all streams must cover the same series list");
    HIP_TRY(hipSetDevice(ctx->device));

    CmPlan pl;
    pl.nseries = nseries;
    GsStatus st = cm_plan_ranks(ctx, sets, nsets, d_ts, pl);
    /* an unsorted stream is known once the flags kernel has run */
    if (st == GS_OK) st = check_dev_err(ctx);
    const int64_t nout = st == GS_OK ? pl.ooff[nseries] : 0;
    if (st == GS_OK && nstr > 0 &&
        nout > int64_t(SCAN_BLOCK) * SCAN_ITEMS * 131072)
        st = bad(GS_ERR, "string merge row limit exceeded (268M)");
    if (st != GS_OK) {
        hipStreamSynchronize(ctx->stream);
        pl.release();
        return st;
    }
    auto dalloc = [&](size_t bytes) -> void * {
        void *q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 1) != hipSuccess) return nullptr;
        pl.scratch.push_back(q);
        return q;
    };
    auto oom = [&]() {
        hipStreamSynchronize(ctx->stream);
        pl.release();
        return bad(GS_ERR, "hipMalloc merge scratch failed");
    };

    /* string columns: one reference array per stream, one reference
       column of the output per string column */
    uint64_t *d_ref[GS_MAX_STREAMS] = {};
    std::vector<uint64_t *> d_refout(nstr, nullptr);
    if (nstr > 0) {
        for (int f = 0; f < nsets; f++) {
            const int64_t rows = sets[f]->total_rows;
            if (!(d_ref[f] = (uint64_t *)dalloc(size_t(rows) * 8))) return oom();
            hipLaunchKernelGGL(k_cm_str_refs, dim3(grid_for(rows, 256)),
                               dim3(256), 0, ctx->stream, d_ref[f], rows, f);
        }
        for (int c = 0; c < nstr; c++)
            if (!(d_refout[c] = (uint64_t *)dalloc(size_t(nout) * 8)))
                return oom();
    }

    /* device pointer table: val | valid | out_val | out_valid */
    const size_t ncell = size_t(nsets) * nc;
    std::vector<const void *> tab(2 * ncell + 2 * size_t(nc), nullptr);
    for (int f = 0; f < nsets; f++) {
        for (int c = 0; c < ncols; c++) {
            tab[f * nc + c] = d_val[f * ncols + c];
            tab[ncell + f * nc + c] = d_valid ? d_valid[f * ncols + c] : nullptr;
        }
        for (int c = 0; c < nstr; c++) {
            const GsStrColumn &in = str_in[f * nstr + c];
            tab[f * nc + ncols + c] = in.d_offsets ? d_ref[f] : nullptr;
            tab[ncell + f * nc + ncols + c] = in.d_valid;
        }
    }
    for (int c = 0; c < ncols; c++) {
        tab[2 * ncell + c] = d_out_val[c];
        tab[2 * ncell + nc + c] = d_out_valid ? d_out_valid[c] : nullptr;
    }
    for (int c = 0; c < nstr; c++) {
        tab[2 * ncell + ncols + c] = d_refout[c];
        tab[2 * ncell + nc + ncols + c] = str_out[c].d_valid;
    }
    const void **d_tab = (const void **)dalloc(tab.size() * sizeof(void *));
    if (!d_tab) return oom();
    hipError_t he = hipMemcpyAsync(d_tab, tab.data(),
                                   tab.size() * sizeof(void *),
                                   hipMemcpyHostToDevice, ctx->stream);
    if (he == hipSuccess) {
        CompactFieldsArgs fa;
        fa.m = pl.a;
        fa.val = d_tab;
        fa.valid = (const uint8_t *const *)(d_tab + ncell);
        fa.out_val = (void *const *)(d_tab + 2 * ncell);
        fa.out_valid = (uint8_t *const *)(d_tab + 2 * ncell + nc);
        fa.wide = wide;
        fa.ncols = nc;
        hipLaunchKernelGGL(k_cm_scatter_fields, dim3(pl.gx, nsets), dim3(256),
                           0, ctx->stream, fa, nsets, nseries, d_out_ts);
    }
    hipError_t hs = hipStreamSynchronize(ctx->stream);
    if (he != hipSuccess || hs != hipSuccess) pl.release();
    HIP_TRY(he);
    HIP_TRY(hs);

    /* string columns: lengths, offsets scan, capacity check, gather */
    st = GS_OK;
    if (nstr > 0) {
        const int n = int(nout);
        const int nblocks = (n + SCAN_BLOCK * SCAN_ITEMS - 1) /
                            (SCAN_BLOCK * SCAN_ITEMS);
        int64_t *d_len = (int64_t *)dalloc(size_t(n) * 8);
        int64_t *d_bsums = (int64_t *)dalloc((size_t(nblocks) + 1) * 8);
        if (!d_len || !d_bsums) return oom();
        std::vector<CmStrSrc> srcs(nstr);
        for (int c = 0; c < nstr; c++) {
            for (int f = 0; f < GS_MAX_STREAMS; f++) {
                const bool in = f < nsets;
                srcs[c].off[f] = in ? str_in[f * nstr + c].d_offsets : nullptr;
                srcs[c].bytes[f] = in ? str_in[f * nstr + c].d_bytes : nullptr;
            }
            int64_t *off = str_out[c].d_offsets;
            if (n == 0) {
                hipMemsetAsync(off, 0, 8, ctx->stream);
                continue;
            }
            hipLaunchKernelGGL(k_cm_str_lens, dim3(grid_for(n, 256)), dim3(256),
                               0, ctx->stream, srcs[c], d_refout[c],
                               int64_t(n), d_len);
            hipLaunchKernelGGL(k_scan_partials, dim3(nblocks), dim3(SCAN_BLOCK),
                               0, ctx->stream, d_len, n, off, d_bsums);
            hipLaunchKernelGGL(k_scan_fixup, dim3(1), dim3(64), 0, ctx->stream,
                               n, off, d_bsums, nblocks);
            hipLaunchKernelGGL(k_scan_add, dim3(grid_for(n, 256)), dim3(256), 0,
                               ctx->stream, n, off, d_bsums);
        }
        std::vector<int64_t> totals(nstr, 0);
        for (int c = 0; c < nstr; c++)
            hipMemcpyAsync(&totals[c], str_out[c].d_offsets + n, 8,
                           hipMemcpyDeviceToHost, ctx->stream);
        hs = hipStreamSynchronize(ctx->stream);
        if (hs != hipSuccess) pl.release();
        HIP_TRY(hs);
        for (int c = 0; c < nstr; c++) {
            str_out[c].total_bytes = totals[c];
            if (totals[c] > str_out[c].bytes_cap)
                st = bad(GS_ERR_CAP, "a string column's bytes_cap is below "
                                     "its total_bytes");
        }
        if (st == GS_OK && n > 0) {
            for (int c = 0; c < nstr; c++)
                hipLaunchKernelGGL(k_cm_str_gather, dim3(grid_for(n, 256)),
                                   dim3(256), 0, ctx->stream, srcs[c],
                                   d_refout[c], str_out[c].d_offsets,
                                   int64_t(n), str_out[c].d_bytes);
            hs = hipStreamSynchronize(ctx->stream);
            if (hs != hipSuccess) pl.release();
            HIP_TRY(hs);
        }
    }
    pl.release();
    if (h_out_offsets)
        memcpy(h_out_offsets, pl.ooff.data(), size_t(nseries + 1) * 8);
    if (out_rows) *out_rows = nout;
    return st;
}
} // namespace

GsStatus gs_compact_merge_fields(GsCtx *ctx, GsGroupSet *const *sets,
                                 int32_t nsets, int32_t ncols,
                                 const int32_t *elem_size,
                                 const int64_t *const *d_ts,
                                 const void *const *d_val,
                                 const uint8_t *const *d_valid,
                                 int64_t *d_out_ts, void *const *d_out_val,
                                 uint8_t *const *d_out_valid,
                                 int64_t *h_out_offsets, int64_t *out_rows) {
    if (!ctx || !sets || !elem_size || !d_ts || !d_val || !d_out_ts ||
        !d_out_val)
        return fail(GS_ERR, "bad args to gs_compact_merge_fields");
    if (ncols < 1)
        return fail(GS_ERR, "gs_compact_merge_fields: ncols outside "
                            "1..GS_MAX_MERGE_COLS");
    return cm_merge_group(ctx, sets, nsets, ncols, elem_size, d_ts, d_val,
                          d_valid, 0, nullptr, d_out_ts, d_out_val,
                          d_out_valid, nullptr, h_out_offsets, out_rows,
                          "gs_compact_merge_fields");
}

GsStatus gs_compact_merge_group(GsCtx *ctx, GsGroupSet *const *sets,
                                int32_t nsets, int32_t ncols,
                                const int32_t *elem_size,
                                const int64_t *const *d_ts,
                                const void *const *d_val,
                                const uint8_t *const *d_valid, int32_t nstr,
                                const GsStrColumn *str_in, int64_t *d_out_ts,
                                void *const *d_out_val,
                                uint8_t *const *d_out_valid,
                                GsStrColumnOut *str_out,
                                int64_t *h_out_offsets, int64_t *out_rows) {
    return cm_merge_group(ctx, sets, nsets, ncols, elem_size, d_ts, d_val,
                          d_valid, nstr, str_in, d_out_ts, d_out_val,
                          d_out_valid, str_out, h_out_offsets, out_rows,
                          "gs_compact_merge_group");
}

/* the one-column case of gs_compact_merge_fields: the per-stream d_val and
 * d_valid arrays are its [nsets*1] tables */
GsStatus gs_compact_merge(GsCtx *ctx, GsGroupSet *const *sets, int32_t nsets,
                          const int64_t *const *d_ts,
                          const double *const *d_val,
                          const uint8_t *const *d_valid, int64_t *d_out_ts,
                          double *d_out_val, uint8_t *d_out_valid,
                          int64_t *h_out_offsets, int64_t *out_rows) {
    if (!ctx || !sets || nsets < 1 || nsets > GS_MAX_STREAMS || !d_ts ||
        !d_val || !d_out_ts || !d_out_val)
        return fail(GS_ERR, "bad args to gs_compact_merge");
    const int32_t elem_size = 8;
    void *const out_val = d_out_val;
    uint8_t *const out_valid = d_out_valid;
    return gs_compact_merge_fields(ctx, sets, nsets, 1, &elem_size, d_ts,
                                   (const void *const *)d_val, d_valid,
                                   d_out_ts, &out_val, &out_valid,
                                   h_out_offsets, out_rows);
}

/* ---- DataFilter over a column group (see cnosdb_gs.h) ---- */

/* debug: device time of the last gs_filter_group call, mask kernel to last
   kernel, from HIP events on the engine stream (the probe's like-for-like
   figure against GsScanResult.ms_filter + ms_compact) */
static std::atomic<float> g_flt_ms{0.f};
float gs_debug_filter_ms(void) {
    return g_flt_ms.load(std::memory_order_relaxed);
}
/* debug: rows per block of the filter kernels, for the tests' edge sizes */
int32_t gs_debug_filter_tile(void) { return FLT_TILE; }

} // extern "C"

namespace {
/* What gs_filter_group and gs_agg_group share in front of their kernels:
 * the argument checks of the filter and its columns, every range list in
 * normal form in one table (row tombstones first) and the columns as the
 * kernels see them.  `who` names the entry in messages; `outputs` is false
 * for gs_agg_group, which ignores the output fields of the columns. */
struct FltPlan {
    std::vector<GsTimeRange> rtab;
    std::vector<FltCol> fc;   /* [ncols + nstr] */
    std::vector<int> pstr;    /* projected string columns */
    int32_t row_cnt = 0;
    int64_t nseg = 0;
};

GsStatus flt_plan(const char *who, bool outputs, const GsGroupSet *set,
                  const GsFilterSpec *spec, int32_t ncols,
                  const GsFilterCol *cols, int32_t nstr,
                  const GsFilterStrCol *strs, FltPlan &pl) {
    auto bad = [who](const char *msg) {
        return fail(GS_ERR, (std::string(who) + ": " + msg).c_str());
    };
    if (ncols < 0 || nstr < 0 || ncols > GS_MAX_MERGE_COLS ||
        nstr > GS_MAX_MERGE_COLS || ncols + nstr < 1 ||
        ncols + nstr > GS_MAX_MERGE_COLS)
        return bad("ncols + nstr outside 1..GS_MAX_MERGE_COLS");
    const int npreds = spec->npreds;
    if (npreds < 0 || npreds > GS_MAX_FILTER_PREDS)
        return bad("npreds outside 0..GS_MAX_FILTER_PREDS");
    if ((ncols > 0 && !cols) || (nstr > 0 && !strs) ||
        (npreds > 0 && !spec->preds) ||
        (spec->n_row_tombstones > 0 && !spec->row_tombstones))
        return bad("NULL argument");
    size_t nranges_in = spec->n_row_tombstones;
    for (int c = 0; c < ncols; c++) {
        const uint8_t ct = cols[c].ctype;
        if (ct != GS_CT_I64 && ct != GS_CT_F64 && ct != GS_CT_BOOL &&
            ct != GS_CT_U64)
            return bad("column ctype must be i64, f64, bool or u64");
        if (!cols[c].d_val || (cols[c].n_tombstones > 0 && !cols[c].tombstones))
            return bad("NULL column pointer");
        nranges_in += cols[c].n_tombstones;
    }
    for (int c = 0; c < nstr; c++) {
        if (strs[c].n_tombstones > 0 && !strs[c].tombstones)
            return bad("NULL column pointer");
        const GsStrColumnOut *o = outputs ? strs[c].out : nullptr;
        if (o && (!strs[c].in.d_offsets || !strs[c].in.d_bytes ||
                  !o->d_offsets || !o->d_bytes || o->bytes_cap < 0))
            return bad("NULL string column pointer");
        nranges_in += strs[c].n_tombstones;
    }
    if (nranges_in > size_t(1) << 30) return bad("too many tombstone ranges");
    for (int p = 0; p < npreds; p++) {
        const GsColPred &pr = spec->preds[p];
        if (!flt_op_known(pr.op)) return bad("unknown predicate op");
        if (pr.col < 0 || pr.col >= ncols + nstr)
            return bad("predicate column out of range");
        if (pr.col >= ncols && !flt_op_is_null_test(pr.op))
            return bad("a string column takes IS_NULL / IS_NOT_NULL only");
    }
    const int64_t rows = set->total_rows;
    if (outputs && nstr > 0 && rows > (int64_t(1) << 28))
        return bad("string column row limit exceeded (2^28)");
    pl.nseg = (rows + FLT_SEG - 1) / FLT_SEG;
    if (pl.nseg > INT32_MAX / 2)
        return bad("too many rows for the segment scan");

    /* every range list in normal form, one table: row tombstones first */
    std::vector<GsTimeRange> &rtab = pl.rtab;
    rtab.clear();
    rtab.reserve(nranges_in);
    auto add_list = [&](const GsTimeRange *r, size_t n, int32_t &off,
                        int32_t &cnt) {
        off = int32_t(rtab.size());
        rtab.insert(rtab.end(), r, r + n);
        cnt = int32_t(flt_normalise(rtab.data() + off, int64_t(n)));
        rtab.resize(size_t(off) + size_t(cnt));
    };
    int32_t row_off0 = 0;
    add_list(spec->row_tombstones, spec->n_row_tombstones, row_off0,
             pl.row_cnt);
    std::vector<FltCol> &fc = pl.fc;
    fc.assign(size_t(ncols + nstr), FltCol());
    for (int c = 0; c < ncols; c++) {
        FltCol &f = fc[c];
        f.val = cols[c].d_val;
        f.valid = cols[c].d_valid;
        f.out_val = outputs ? cols[c].d_out_val : nullptr;
        f.out_valid = f.out_val ? cols[c].d_out_valid : nullptr;
        f.ctype = cols[c].ctype;
        f.pad = 0;
        add_list(cols[c].tombstones, cols[c].n_tombstones, f.rng_off,
                 f.rng_cnt);
    }
    pl.pstr.clear();
    for (int c = 0; c < nstr; c++) {
        FltCol &f = fc[ncols + c];
        const GsStrColumnOut *o = outputs ? strs[c].out : nullptr;
        f.val = nullptr;
        f.valid = strs[c].in.d_valid;
        f.out_val = nullptr; /* its reference array, set by the entry */
        f.out_valid = o ? o->d_valid : nullptr;
        f.ctype = GS_CT_STR;
        f.pad = 0;
        add_list(strs[c].tombstones, strs[c].n_tombstones, f.rng_off,
                 f.rng_cnt);
        if (o) pl.pstr.push_back(c);
    }
    return GS_OK;
}

/* the range table into the set's cached device copy, and the mask kernel's
   arguments; call after hipSetDevice */
GsStatus flt_mask_args(GsCtx *ctx, GsGroupSet *set, const int64_t *d_ts,
                       const GsFilterSpec *spec, const FltPlan &pl,
                       FltMaskArgs &ma) {
    if (set->flt_ranges_cap < pl.rtab.size()) {
        if (set->d_flt_ranges) hipFree(set->d_flt_ranges);
        set->d_flt_ranges = nullptr;
        set->flt_ranges_cap = 0;
        HIP_TRY(hipMalloc(&set->d_flt_ranges,
                          pl.rtab.size() * sizeof(GsTimeRange)));
        set->flt_ranges_cap = pl.rtab.size();
    }
    if (!pl.rtab.empty())
        HIP_TRY(hipMemcpyAsync(set->d_flt_ranges, pl.rtab.data(),
                               pl.rtab.size() * sizeof(GsTimeRange),
                               hipMemcpyHostToDevice, ctx->stream));
    memset(&ma, 0, sizeof(ma));
    ma.ts = d_ts;
    ma.ranges = set->d_flt_ranges;
    ma.rows = set->total_rows;
    ma.lo = spec->range.min_ts;
    ma.hi = spec->range.max_ts;
    ma.row_rng_cnt = pl.row_cnt;
    ma.npreds = spec->npreds;
    for (int p = 0; p < spec->npreds; p++) {
        ma.pred[p] = spec->preds[p];
        ma.pcol[p] = pl.fc[spec->preds[p].col];
    }
    return GS_OK;
}
} // namespace

extern "C" {

GsStatus gs_filter_group(GsCtx *ctx, GsGroupSet *set, const int64_t *d_ts,
                         const GsFilterSpec *spec, int32_t ncols,
                         const GsFilterCol *cols, int32_t nstr,
                         const GsFilterStrCol *strs, int64_t *d_out_ts,
                         int64_t *h_out_offsets, int64_t *out_rows) {
    auto bad = [](const char *msg) {
        return fail(GS_ERR, (std::string("gs_filter_group: ") + msg).c_str());
    };
    if (!ctx || !set || !d_ts || !spec || !d_out_ts || !h_out_offsets ||
        !out_rows)
        return bad("NULL argument");
    FltPlan pl;
    if (GsStatus st0 = flt_plan("gs_filter_group", true, set, spec, ncols,
                                cols, nstr, strs, pl))
        return st0;
    std::vector<FltCol> &fc = pl.fc;
    const std::vector<int> &pstr = pl.pstr;
    const int64_t rows = set->total_rows;
    const int ng = int(set->ngroups);
    const int64_t nseg = pl.nseg;

    HIP_TRY(hipSetDevice(ctx->device));
    if (rows == 0) {
        for (int c : pstr) {
            HIP_TRY(hipMemsetAsync(strs[c].out->d_offsets, 0, 8, ctx->stream));
            strs[c].out->total_bytes = 0;
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (int g = 0; g <= ng; g++) h_out_offsets[g] = 0;
        *out_rows = 0;
        return GS_OK;
    }

    /* scratch, cached in the set */
    const int64_t scan_chunk = int64_t(SCAN_BLOCK) * SCAN_ITEMS;
    const int64_t seg_blocks = (nseg + scan_chunk - 1) / scan_chunk;
    if (!set->d_mask) HIP_TRY(hipMalloc(&set->d_mask, size_t(rows)));
    if (!set->d_flt_seg)
        HIP_TRY(hipMalloc(&set->d_flt_seg,
                          size_t(2 * nseg + 1 + seg_blocks + 1) * 8));
    int64_t *d_seg_cnt = set->d_flt_seg;
    int64_t *d_seg_off = d_seg_cnt + nseg;        /* [nseg + 1] */
    int64_t *d_seg_bsums = d_seg_off + nseg + 1;  /* [seg_blocks + 1] */
    /* per projected string column a reference array, then the lengths and
       the offset scan's block sums */
    const int64_t row_blocks = (rows + scan_chunk - 1) / scan_chunk;
    const size_t ref_need =
        pstr.empty() ? 0
                     : (pstr.size() + 1) * size_t(rows) + size_t(row_blocks) + 1;
    if (set->flt_ref_cap < ref_need) {
        if (set->d_flt_ref) hipFree(set->d_flt_ref);
        set->d_flt_ref = nullptr;
        set->flt_ref_cap = 0;
        HIP_TRY(hipMalloc(&set->d_flt_ref, ref_need * 8));
        set->flt_ref_cap = ref_need;
    }
    for (size_t k = 0; k < pstr.size(); k++)
        fc[ncols + pstr[k]].out_val = set->d_flt_ref + k * size_t(rows);

    hipEvent_t ev[2];
    HIP_TRY(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) {
        hipEventDestroy(ev[0]);
        return bad("hipEventCreate failed");
    }
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard() { hipEventDestroy(e[0]); hipEventDestroy(e[1]); }
    } guard{ev};

    FltMaskArgs ma;
    if (GsStatus st0 = flt_mask_args(ctx, set, d_ts, spec, pl, ma)) return st0;
    FltGatherArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.ts = d_ts;
    ga.ranges = set->d_flt_ranges;
    ga.rows = rows;
    for (const FltCol &f : fc)
        if (f.out_val) ga.col[ga.ncol++] = f;

    const int64_t ntile = (nseg + 3) / 4;
    HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    hipLaunchKernelGGL(k_flt_mask, dim3(grid_items(ntile, 2048)), dim3(256), 0,
                       ctx->stream, ma, nseg, set->d_mask, d_seg_cnt);
    {
        const int n = int(nseg);
        const int nblocks = int(seg_blocks);
        hipLaunchKernelGGL(k_scan_partials, dim3(nblocks), dim3(SCAN_BLOCK), 0,
                           ctx->stream, d_seg_cnt, n, d_seg_off, d_seg_bsums);
        hipLaunchKernelGGL(k_scan_fixup, dim3(1), dim3(64), 0, ctx->stream, n,
                           d_seg_off, d_seg_bsums, nblocks);
        hipLaunchKernelGGL(k_scan_add, dim3(grid_for(n, 256)), dim3(256), 0,
                           ctx->stream, n, d_seg_off, d_seg_bsums);
    }
    hipLaunchKernelGGL(k_flt_gather, dim3(grid_items(ntile, 2048)), dim3(256),
                       0, ctx->stream, ga, nseg, set->d_mask, d_seg_off,
                       d_out_ts);
    hipLaunchKernelGGL(k_flt_group_off,
                       dim3(grid_for((int64_t(ng) + 1) * 64, 256)), dim3(256),
                       0, ctx->stream, set->d_groups, ng, rows, set->d_mask,
                       d_seg_off, nseg, set->d_out_off);
    HIP_TRY(hipEventRecord(ev[1], ctx->stream));
    HIP_TRY(hipMemcpyAsync(h_out_offsets, set->d_out_off,
                           (size_t(ng) + 1) * 8, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int64_t nout = h_out_offsets[ng];
    *out_rows = nout;

    /* string columns: lengths, offsets scan, capacity check, gather — the
       kernels of gs_compact_merge_group over one stream */
    GsStatus st = GS_OK;
    if (!pstr.empty()) {
        const int n = int(nout);
        const int nblocks = int((nout + scan_chunk - 1) / scan_chunk);
        int64_t *d_len = (int64_t *)(set->d_flt_ref + pstr.size() * size_t(rows));
        int64_t *d_bsums = d_len + rows;
        std::vector<CmStrSrc> srcs(pstr.size());
        std::vector<int64_t> totals(pstr.size(), 0);
        for (size_t k = 0; k < pstr.size(); k++) {
            const GsFilterStrCol &sc = strs[pstr[k]];
            memset(&srcs[k], 0, sizeof(CmStrSrc));
            srcs[k].off[0] = sc.in.d_offsets;
            srcs[k].bytes[0] = sc.in.d_bytes;
            int64_t *off = sc.out->d_offsets;
            const uint64_t *ref = set->d_flt_ref + k * size_t(rows);
            if (n == 0) {
                HIP_TRY(hipMemsetAsync(off, 0, 8, ctx->stream));
                continue;
            }
            hipLaunchKernelGGL(k_cm_str_lens, dim3(grid_for(n, 256)), dim3(256),
                               0, ctx->stream, srcs[k], ref, int64_t(n), d_len);
            hipLaunchKernelGGL(k_scan_partials, dim3(nblocks), dim3(SCAN_BLOCK),
                               0, ctx->stream, d_len, n, off, d_bsums);
            hipLaunchKernelGGL(k_scan_fixup, dim3(1), dim3(64), 0, ctx->stream,
                               n, off, d_bsums, nblocks);
            hipLaunchKernelGGL(k_scan_add, dim3(grid_for(n, 256)), dim3(256), 0,
                               ctx->stream, n, off, d_bsums);
            HIP_TRY(hipMemcpyAsync(&totals[k], off + n, 8,
                                   hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        for (size_t k = 0; k < pstr.size(); k++) {
            GsStrColumnOut *o = strs[pstr[k]].out;
            o->total_bytes = totals[k];
            if (totals[k] > o->bytes_cap)
                st = fail(GS_ERR_CAP, "gs_filter_group: a string column's "
                                      "bytes_cap is below its total_bytes");
        }
        if (st == GS_OK && n > 0) {
            for (size_t k = 0; k < pstr.size(); k++)
                hipLaunchKernelGGL(k_cm_str_gather, dim3(grid_for(n, 256)),
                                   dim3(256), 0, ctx->stream, srcs[k],
                                   set->d_flt_ref + k * size_t(rows),
                                   strs[pstr[k]].out->d_offsets, int64_t(n),
                                   strs[pstr[k]].out->d_bytes);
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
        g_flt_ms.store(ms, std::memory_order_relaxed);
    return st;
}

/* ---- typed bucket aggregates over a filtered column group (see
 * cnosdb_gs.h) ---- */

/* debug: device time of the last gs_agg_group call, first to last kernel,
   from HIP events on the engine stream */
static std::atomic<float> g_agg_ms{0.f};
float gs_debug_agg_ms(void) {
    return g_agg_ms.load(std::memory_order_relaxed);
}

GsStatus gs_agg_group(GsCtx *ctx, GsGroupSet *set, const int64_t *d_ts,
                      const GsFilterSpec *filter, int32_t ncols,
                      const GsFilterCol *cols, int32_t nstr,
                      const GsFilterStrCol *strs, const GsAggSpec *agg,
                      int32_t naggs, const GsAggOut *outs, int64_t *d_rows) {
    auto bad = [](const char *msg) {
        return fail(GS_ERR, (std::string("gs_agg_group: ") + msg).c_str());
    };
    if (!ctx || !set || !d_ts || !filter || !agg) return bad("NULL argument");
    FltPlan pl;
    if (GsStatus st0 = flt_plan("gs_agg_group", false, set, filter, ncols,
                                cols, nstr, strs, pl))
        return st0;
    if (naggs < 1 || naggs > GS_MAX_MERGE_COLS)
        return bad("naggs outside 1..GS_MAX_MERGE_COLS");
    if (!outs) return bad("NULL argument");
    for (int i = 0; i < naggs; i++)
        if (outs[i].col < 0 || outs[i].col >= ncols)
            return bad("aggregated column out of range (fixed-width columns "
                       "only)");
    if (agg->n_buckets < 1) return bad("n_buckets < 1");
    if (agg->bucket_ns < 0) return bad("bucket_ns < 0");
    if (agg->bucket_ns == 0 && agg->n_buckets != 1)
        return bad("bucket_ns == 0 takes n_buckets == 1");
    const int64_t rows = set->total_rows;
    const int nsg = set->nsgroups;
    const int64_t scells = int64_t(nsg) * agg->n_buckets;
    const bool per_series = agg->per_series != 0;
    const int64_t cells = per_series ? scells : int64_t(agg->n_buckets);
    if (cells > INT32_MAX) return bad("more than 2^31 - 1 cells");
    const int ncol = naggs + (d_rows ? 1 : 0);
    const int64_t nseg = pl.nseg, nrec = 2 * nseg;

    HIP_TRY(hipSetDevice(ctx->device));
    /* the column table: the aggregated columns, then the row counter */
    std::vector<AggCol> hc;
    hc.resize(size_t(ncol));
    memset(hc.data(), 0, hc.size() * sizeof(AggCol));
    for (int i = 0; i < naggs; i++) {
        AggCol &c = hc[i];
        c.c = pl.fc[outs[i].col];
        c.o_count = outs[i].d_count;
        c.o_sum = outs[i].d_sum;
        c.o_mn = outs[i].d_min;
        c.o_mx = outs[i].d_max;
        c.o_first = outs[i].d_first;
        c.o_last = outs[i].d_last;
        c.o_first_ts = outs[i].d_first_ts;
        c.o_last_ts = outs[i].d_last_ts;
    }
    if (d_rows) {
        hc[naggs].c.ctype = GS_CT_TIME; /* val NULL: every kept row counts */
        hc[naggs].o_count = d_rows;
    }
    if (!set->d_agg_cols)
        HIP_TRY(hipMalloc(&set->d_agg_cols,
                          (GS_MAX_MERGE_COLS + 1) * sizeof(AggCol)));
    auto grow = [](uint64_t *&p, size_t &cap, size_t need) {
        if (cap >= need) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipMalloc(&p, need * 8);
        if (e == hipSuccess) cap = need;
        return e;
    };
    HIP_TRY(grow(set->d_agg_carry, set->agg_carry_cap,
                 size_t(nrec) * (1 + size_t(AGG_NFIELD) * ncol)));
    if (!per_series)
        HIP_TRY(grow(set->d_agg_scr, set->agg_scr_cap,
                     size_t(scells) * AGG_NFIELD * ncol));

    hipEvent_t ev[2];
    HIP_TRY(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) {
        hipEventDestroy(ev[0]);
        return bad("hipEventCreate failed");
    }
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard() { hipEventDestroy(e[0]); hipEventDestroy(e[1]); }
    } guard{ev};

    FltMaskArgs ma;
    if (GsStatus st0 = flt_mask_args(ctx, set, d_ts, filter, pl, ma))
        return st0;
    const AggCol *d_cols = (const AggCol *)set->d_agg_cols;
    HIP_TRY(hipMemcpyAsync(set->d_agg_cols, hc.data(),
                           hc.size() * sizeof(AggCol), hipMemcpyHostToDevice,
                           ctx->stream));
    AggGeom g;
    memset(&g, 0, sizeof(g));
    g.sg = set->d_sgroups;
    g.nsg = nsg;
    g.nb = agg->n_buckets;
    g.t0 = agg->t0;
    g.bn = agg->bucket_ns;
    g.ncol = ncol;
    g.scratch = per_series ? nullptr : set->d_agg_scr;
    g.scells = scells;
    g.ckey = (int64_t *)set->d_agg_carry;
    g.ctab = set->d_agg_carry + nrec;
    g.nrec = nrec;

    HIP_TRY(hipEventRecord(ev[0], ctx->stream));
    hipLaunchKernelGGL(k_agg_init,
                       dim3(grid_for(per_series ? cells : scells, 256)),
                       dim3(256), 0, ctx->stream, g, d_cols, cells);
    if (nseg > 0) {
        const int64_t ntile = (nseg + 3) / 4;
        hipLaunchKernelGGL(k_agg_seg, dim3(grid_items(ntile, 2048)), dim3(256),
                           0, ctx->stream, ma, g, d_cols, nseg, ctx->d_err);
        hipLaunchKernelGGL(k_agg_stitch, dim3(grid_for(nrec * ncol * 64, 256)),
                           dim3(256), 0, ctx->stream, g, d_cols);
    }
    if (!per_series)
        hipLaunchKernelGGL(k_agg_fold,
                           dim3(grid_for(int64_t(g.nb) * ncol * 64, 256)),
                           dim3(256), 0, ctx->stream, g, d_cols);
    HIP_TRY(hipEventRecord(ev[1], ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess)
        g_agg_ms.store(ms, std::memory_order_relaxed);
    unsigned e = 0;
    HIP_TRY(hipMemcpy(&e, ctx->d_err, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (e) {
        hipMemset(ctx->d_err, 0, sizeof(unsigned));
        return fail(GS_ERR_FORMAT, "gs_agg_group: timestamps do not strictly "
                                   "increase inside a series");
    }
    return GS_OK;
}

/* ---- Arrow C Data Interface export ---- */
namespace {
struct ExportPriv {
    void *data;
    uint8_t *bitmap;
    const void *bufs[2];
};
void export_release(GsArrowArray *a) {
    if (!a || !a->private_data) return;
    ExportPriv *p = (ExportPriv *)a->private_data;
    free(p->data);
    free(p->bitmap);
    free(p);
    a->release = nullptr;
    a->private_data = nullptr;
}
} // namespace

GsStatus gs_export_group_column(GsCtx *ctx, GsGroupSet *set, int64_t group,
                                const void *d_col, int32_t elem_size,
                                const uint8_t *d_valid, GsArrowArray *out) {
    if (!ctx || !set || group < 0 || size_t(group) >= set->ngroups || !d_col ||
        !out || (elem_size != 8 && elem_size != 1))
        return fail(GS_ERR, "bad args to gs_export_group_column");
    HIP_TRY(hipSetDevice(ctx->device));
    int64_t row0 = set->row_offsets[group];
    int64_t rows = (size_t(group) + 1 < set->ngroups
                        ? set->row_offsets[group + 1]
                        : set->total_rows) - row0;
    ExportPriv *p = (ExportPriv *)calloc(1, sizeof(ExportPriv));
    if (!p) return fail(GS_ERR, "oom");
    p->data = malloc(size_t(rows) * elem_size ? size_t(rows) * elem_size : 1);
    if (!p->data) { free(p); return fail(GS_ERR, "oom"); }
    if (hipMemcpy(p->data, (const uint8_t *)d_col + row0 * elem_size,
                  size_t(rows) * elem_size, hipMemcpyDeviceToHost) !=
        hipSuccess) {
        free(p->data); free(p);
        return fail(GS_ERR, "export D2H failed");
    }
    int64_t null_count = 0;
    if (d_valid) {
        std::vector<uint8_t> vbytes(rows);
        if (hipMemcpy(vbytes.data(), d_valid + row0, size_t(rows),
                      hipMemcpyDeviceToHost) != hipSuccess) {
            free(p->data); free(p);
            return fail(GS_ERR, "export validity D2H failed");
        }
        size_t nb = size_t(rows + 7) / 8;
        p->bitmap = (uint8_t *)calloc(nb ? nb : 1, 1);
        if (!p->bitmap) { free(p->data); free(p); return fail(GS_ERR, "oom"); }
        for (int64_t r = 0; r < rows; r++) {
            if (vbytes[r]) p->bitmap[r >> 3] |= uint8_t(1u << (r & 7));
            else null_count++;
        }
    }
    p->bufs[0] = p->bitmap; /* NULL when no validity buffer */
    p->bufs[1] = p->data;
    out->length = rows;
    out->null_count = d_valid ? null_count : 0;
    out->offset = 0;
    out->n_buffers = 2;
    out->n_children = 0;
    out->buffers = p->bufs;
    out->children = nullptr;
    out->dictionary = nullptr;
    out->release = export_release;
    out->private_data = p;
    return GS_OK;
}

} // extern "C"
