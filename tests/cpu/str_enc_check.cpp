/* Stand-alone host check of cnosdb_amd/csrc/gs_str_enc.h, built with
 * -fsanitize=address,undefined by tests/test_str_enc_cpu.py.  The header is
 * compiled with STR_ENC_BYTE_LOADS, i.e. with the loads and copies the
 * device kernel k_str_enc_pages runs.  Every case is encoded from a heap
 * payload block of exactly the payload's size, through a heap hash table of
 * exactly the entries in use, into a heap block of exactly
 * str_enc_max_len(payload) bytes, so any access outside what the encoder is
 * entitled to stops the program; the result is compared with the expected
 * block of the case file (the oracle's).
 *
 * Case file (little-endian):
 *   u32 ncases
 *   per case: u32 name_len, name; u32 nstr; nstr x u64 length; the strings
 *             back to back; u32 block_len; block
 * Prints "N cases, F failures"; exit status 1 if F > 0. */
#define STR_ENC_BYTE_LOADS 1
#include "gs_str_enc.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

static_assert(STR_ENC_BYTEWISE == 1, "the device's loads are under test");

static bool read_exact(FILE *f, void *dst, size_t n) {
    return n == 0 || fread(dst, 1, n, f) == n;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4)) return 2;
    int failures = 0;
    for (uint32_t c = 0; c < ncases; c++) {
        uint32_t name_len = 0, nstr = 0, block_len = 0;
        if (!read_exact(f, &name_len, 4)) return 2;
        std::string name(name_len, '\0');
        if (!read_exact(f, &name[0], name_len) || !read_exact(f, &nstr, 4))
            return 2;
        std::unique_ptr<uint64_t[]> lens(new uint64_t[nstr]);
        if (!read_exact(f, lens.get(), 8 * size_t(nstr))) return 2;
        uint64_t nbytes = 0;
        for (uint32_t i = 0; i < nstr; i++) nbytes += lens[i];
        std::unique_ptr<uint8_t[]> src(new uint8_t[nbytes]);
        if (!read_exact(f, src.get(), nbytes) || !read_exact(f, &block_len, 4))
            return 2;
        std::unique_ptr<uint8_t[]> want(new uint8_t[block_len]);
        if (!read_exact(f, want.get(), block_len)) return 2;

        int64_t got_len = 0;
        std::unique_ptr<uint8_t[]> dst;
        if (nstr > 0) { /* no strings: the empty block, nothing to run */
            const uint64_t payload = str_enc_payload_len(lens.get(), nstr);
            std::unique_ptr<uint8_t[]> buf(new uint8_t[payload]);
            str_enc_payload(src.get(), lens.get(), nstr, buf.get());
            const uint32_t tsz = str_enc_table_size(
                payload < STR_ENC_FRAGMENT ? size_t(payload) : STR_ENC_FRAGMENT);
            std::unique_ptr<uint16_t[]> tab(new uint16_t[tsz]);
            dst.reset(new uint8_t[str_enc_max_len(payload)]);
            got_len = str_enc_block(buf.get(), payload, dst.get(), tab.get());
            if (uint64_t(got_len) > str_enc_max_len(payload)) got_len = -1;
        }
        const bool ok = got_len == int64_t(block_len) &&
                        (block_len == 0 ||
                         memcmp(dst.get(), want.get(), block_len) == 0);
        if (!ok) {
            failures++;
            printf("FAIL %s: %lld bytes, expected %u\n", name.c_str(),
                   (long long)got_len, block_len);
        }
    }
    fclose(f);
    printf("%u cases, %d failures\n", ncases, failures);
    return failures ? 1 : 0;
}
