/* Host check of the Gorilla window parser (cnosdb_amd/csrc/gs_gorilla.h),
 * built with AddressSanitizer and UBSan by tests/test_gor_window_cpu.py.
 *
 * Input file (little-endian), written by the test:
 *   u32 npages
 *   per page: u32 nvals, u32 data_len, u32 cut,
 *             data_len bytes of page data + the blob's 48 zero pad bytes,
 *             nvals u64 expected bit patterns
 * Every page sits in a heap block of exactly data_len + 48 bytes, so a read
 * past the pad is an ASan error.
 *
 * Whole pages: for chunk sizes 1, 7 and 64 the stream is walked from the
 * page start as k_gor_sync does, recording the state every K values; every
 * recorded state is then resumed and its chunk decoded as k_gor_chunks
 * does; all values are compared bit for bit, and the bit count at the
 * sentinel with the stream's length.  Cut pages: the walk has to end
 * through the overrun flag or a bit count past the stream's end. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "gs_gorilla.h"

struct Page {
    uint32_t nvals, data_len, cut;
    std::unique_ptr<uint8_t[]> data; /* data_len + 48 bytes */
    std::vector<uint64_t> expect;
};

static bool read_exact(FILE *f, void *dst, size_t n) {
    return n == 0 || fread(dst, 1, n, f) == n;
}

/* chunk skeletons as gs_groups_upload builds them (data_off = 0: the page
 * is its own blob) */
static std::vector<DevGorChunk> skeleton(const Page &pg, uint32_t K) {
    uint32_t nch = pg.nvals ? (pg.nvals + K - 1) / K : 1;
    std::vector<DevGorChunk> ch(nch);
    for (uint32_t k = 0; k < nch; k++) {
        DevGorChunk c{};
        c.row0 = k * K;
        c.cnt = pg.nvals > c.row0
                    ? (pg.nvals - c.row0 < K ? pg.nvals - c.row0 : K) : 0;
        c.data_len = pg.data_len;
        c.meaningful = 64;
        c.last = uint8_t(k == nch - 1);
        ch[k] = c;
    }
    return ch;
}

/* k_gor_sync's walk; false = the page would be poisoned */
static bool sync_walk(const Page &pg, uint32_t K,
                      std::vector<DevGorChunk> &ch) {
    const uint32_t nch = uint32_t(ch.size());
    if (nch <= 1) return true;
    GorChunkState st;
    if (!gor_start(st, pg.data.get(), pg.data_len)) return false;
    uint32_t r = 1, next_k = 1;
    for (;;) {
        if (r == next_k * K) {
            if (gor_used_bits(st) > st.total_bits) return false;
            gor_record(st, ch[next_k]);
            if (++next_k == nch) return true;
        }
        if (st.nb < 64) gor_topup(st);
        if (st.over) return false;
        if (gor_parse(st) && st.val == GORILLA_SENTINEL) return false;
        r++;
    }
}

/* k_gor_chunks' decode of one chunk into out[row0 .. row0+cnt); returns
 * nullptr or what went wrong */
static const char *decode_chunk(const Page &pg, const DevGorChunk &c,
                                uint64_t *out) {
    GorChunkState st;
    gor_position(st, pg.data.get(), c);
    if (st.bad) return "positioning failed";
    uint32_t r = c.row0;
    const uint32_t end = c.row0 + c.cnt;
    if (c.row0 == 0 && r < end) out[r++] = st.val; /* header value */
    if (r == end && !c.last) return nullptr; /* K = 1: nothing to parse */
    for (;;) {
        if (st.nb < 64) gor_topup(st);
        if (st.over) return "overrun";
        if (gor_parse(st) && st.val == GORILLA_SENTINEL) {
            if (!c.last) return "sentinel inside a non-last chunk";
            /* the encoder pads the last byte with up to 7 zero bits */
            const int64_t slack = st.total_bits - gor_used_bits(st);
            if (slack < 0 || slack > 7) return "bit count at the sentinel";
            break;
        }
        if (r >= end) return "value after the last row";
        out[r++] = st.val;
        if (r == end && !c.last) {
            if (gor_used_bits(st) > st.total_bits) return "ran past the end";
            break;
        }
    }
    return r < end ? "rows missing" : nullptr;
}

static int check_page(const Page &pg, int pi) {
    int bad = 0;
    for (uint32_t K : {1u, 7u, 64u}) {
        std::vector<DevGorChunk> ch = skeleton(pg, K);
        if (!sync_walk(pg, K, ch)) {
            printf("page %d K=%u: sync walk failed\n", pi, K);
            bad++;
            continue;
        }
        std::vector<uint64_t> got(pg.nvals, 0);
        for (size_t k = 0; k < ch.size(); k++) {
            const char *e = decode_chunk(pg, ch[k], got.data());
            if (e) {
                printf("page %d K=%u chunk %zu: %s\n", pi, K, k, e);
                bad++;
            }
        }
        for (uint32_t i = 0; i < pg.nvals; i++)
            if (got[i] != pg.expect[i]) {
                printf("page %d K=%u row %u: %016llx != %016llx\n", pi, K, i,
                       (unsigned long long)got[i],
                       (unsigned long long)pg.expect[i]);
                bad++;
                break;
            }
    }
    return bad;
}

/* a cut stream: parse as a page's last chunk does, to the sentinel; the
 * zero pad reads as repeats, so only the overrun flag or the bit count can
 * end it */
static int check_cut_page(const Page &pg, int pi) {
    GorChunkState st;
    if (!gor_start(st, pg.data.get(), pg.data_len)) {
        printf("cut page %d: no header\n", pi);
        return 1;
    }
    const int64_t limit = st.total_bits + 1024; /* >= 1 bit per value */
    for (int64_t it = 0; it < limit; it++) {
        if (st.nb < 64) gor_topup(st);
        if (st.over) return 0;
        if (gor_parse(st) && st.val == GORILLA_SENTINEL) {
            if (gor_used_bits(st) > st.total_bits) return 0;
            printf("cut page %d: sentinel inside the stream\n", pi);
            return 1;
        }
    }
    printf("cut page %d: walk did not end\n", pi);
    return 1;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <pages file>\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t npages = 0;
    if (!read_exact(f, &npages, 4)) return 2;
    int bad = 0, nwhole = 0, ncut = 0;
    for (uint32_t pi = 0; pi < npages; pi++) {
        Page pg;
        uint32_t hdr[3];
        if (!read_exact(f, hdr, sizeof(hdr))) return 2;
        pg.nvals = hdr[0];
        pg.data_len = hdr[1];
        pg.cut = hdr[2];
        pg.data.reset(new uint8_t[size_t(pg.data_len) + 48]);
        pg.expect.resize(pg.nvals);
        if (!read_exact(f, pg.data.get(), size_t(pg.data_len) + 48) ||
            !read_exact(f, pg.expect.data(), size_t(pg.nvals) * 8))
            return 2;
        if (pg.cut) { bad += check_cut_page(pg, int(pi)); ncut++; }
        else { bad += check_page(pg, int(pi)); nwhole++; }
    }
    fclose(f);
    printf("%d whole pages, %d cut pages, %d failures\n", nwhole, ncut, bad);
    return bad ? 1 : 0;
}
