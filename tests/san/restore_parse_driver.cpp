// restore_parse_driver.cpp -- stand-alone driver of longtail_amd/csrc/restore_parse.h for tests/test_restore_parse.py: built with
// -fsanitize=address,undefined and run as a program.  It includes the parsing header and nothing else of the library.
//   restore_parse_driver vi|si FILE
// FILE holds a VALID serialized index.  The driver parses, each time from a heap copy of exactly the bytes offered (so that a read past
// them is the sanitizer's to report):
//   the whole blob                                      -> 0
//   every proper prefix                                 -> EBADF
//   each 32-bit header word set to 0xFFFFFFFF           -> EBADF
//   the count words set to values whose array sizes would overflow 32-bit (and, multiplied out carelessly, 64-bit) arithmetic -> EBADF
// and prints "ok <cases>"; the first wrong answer is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../longtail_amd/csrc/restore_parse.h"

static bool g_vi;

static int parse(const std::vector<uint8_t>& blob, size_t size)
{
    uint8_t* copy = (uint8_t*)malloc(size ? size : 1);
    if (size)
        memcpy(copy, blob.data(), size);
    int err;
    if (g_vi)
    {
        restore_parse::VersionIndex v;
        err = restore_parse::parse_version_index(copy, size, &v);
        if (!err)
        {
            uint64_t total = 0;
            std::vector<uint64_t> offs(v.asset_count);
            err = restore_parse::layout(v, 16, offs.data(), &total);
        }
    }
    else
    {
        restore_parse::StoreIndex s;
        err = restore_parse::parse_store_index(copy, size, &s);
    }
    free(copy);
    return err;
}

static int expect(int got, int want, const char* what, uint64_t a, uint64_t b)
{
    if (got == want)
        return 0;
    printf("FAIL %s (%llu, %llu): errno %d, expected %d\n", what, (unsigned long long)a, (unsigned long long)b, got, want);
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 3 || (strcmp(argv[1], "vi") && strcmp(argv[1], "si")))
        return 2;
    g_vi = !strcmp(argv[1], "vi");
    FILE* f = fopen(argv[2], "rb");
    if (!f)
        return 2;
    std::vector<uint8_t> blob;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
        blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    const size_t words = g_vi ? 6 : 4, first_count = g_vi ? 3 : 2;
    if (blob.size() < words * 4)
        return 2;
    uint64_t cases = 0;
    int bad = expect(parse(blob, blob.size()), 0, "the valid blob", blob.size(), 0);
    for (size_t n = 0; n < blob.size() && !bad; ++n, ++cases)
        bad = expect(parse(blob, n), EBADF, "prefix", n, 0);
    for (size_t w = 0; w < words && !bad; ++w, ++cases)
    {
        std::vector<uint8_t> x = blob;
        memset(x.data() + w * 4, 0xFF, 4);
        bad = expect(parse(x, x.size()), EBADF, "header word set to all ones", w, 0);
    }
    // counts whose arrays do not fit the blob, chosen so that 32-bit products wrap to small numbers (0x20000000 * 8 = 0 mod 2^32,
    // 0x40000000 * 4 = 0, 0x80000000 * 2 = 0, 0xAAAAAAAB * 12 = 4) -- alone and all together
    static const uint32_t big[] = {0x20000000u, 0x40000000u, 0x80000000u, 0xAAAAAAABu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (const uint32_t v : big)
    {
        for (size_t w = first_count; w <= words && !bad; ++w, ++cases) // (w == words: every count word)
        {
            std::vector<uint8_t> x = blob;
            for (size_t k = first_count; k < words; ++k)
                if (w == words || w == k)
                    memcpy(x.data() + k * 4, &v, 4);
            bad = expect(parse(x, x.size()), EBADF, "overflowing count", v, w);
        }
    }
    if (bad)
        return 1;
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
