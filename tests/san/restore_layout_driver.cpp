// restore_layout_driver.cpp -- stand-alone driver of longtail_amd/csrc/restore_layout.h (over version_diff.h and restore_parse.h) for
// tests/test_restore_layout_san.py: built with -fsanitize=address,undefined and run as a program.  It includes the header and nothing
// else of the library.
//   restore_layout_driver BASE TARGET OFFSETS BASE_BYTES ALIGN
// BASE and TARGET hold VALID serialized VersionIndexes, OFFSETS the base's asset offsets (uint64 each).  Every blob is offered as a heap
// copy of exactly its bytes (a read past them is the sanitizer's to report):
//   both blobs whole                                    -> 0: "offsets ..." / "total N" / "kept N" printed, one per line
//   the same without an offsets array                   -> 0, the same total and kept
//   every proper prefix of either, the other whole      -> EBADF
//   a null blob, null offsets, ALIGN + 1 (ALIGN > 1), 0 -> EINVAL
// and prints "ok <cases>" last; the first wrong answer is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../longtail_amd/csrc/restore_layout.h"

static std::vector<uint8_t> read_file(const char* path)
{
    std::vector<uint8_t> blob;
    FILE* f = fopen(path, "rb");
    if (!f)
        exit(2);
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
        blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    return blob;
}

struct Answer
{
    std::vector<uint64_t> offsets;
    uint32_t count = 0, kept = 0;
    uint64_t total = 0;
};

static std::vector<uint64_t> g_base_offsets;
static uint64_t g_base_bytes;

static int lay(const std::vector<uint8_t>& a, size_t na, const std::vector<uint8_t>& b, size_t nb, uint64_t align, bool want_offsets, Answer* out)
{
    uint8_t* ca = (uint8_t*)malloc(na ? na : 1);
    uint8_t* cb = (uint8_t*)malloc(nb ? nb : 1);
    if (na)
        memcpy(ca, a.data(), na);
    if (nb)
        memcpy(cb, b.data(), nb);
    // exactly as many offsets as the whole target has assets: a write past them is the sanitizer's to report
    uint32_t assets = 0;
    if (b.size() >= 16)
        memcpy(&assets, b.data() + 12, 4);
    uint64_t* offs = (uint64_t*)malloc(assets ? assets * 8u : 1);
    const int err = restore_layout::in_place(ca, na, g_base_offsets.data(), g_base_bytes, cb, nb, align, want_offsets ? offs : nullptr, &out->count,
                                             &out->total, &out->kept);
    if (!err && want_offsets)
        out->offsets.assign(offs, offs + out->count);
    free(offs);
    free(ca);
    free(cb);
    return err;
}

int main(int argc, char** argv)
{
    if (argc != 6)
        return 2;
    const std::vector<uint8_t> a = read_file(argv[1]), b = read_file(argv[2]), o = read_file(argv[3]);
    g_base_offsets.resize(o.size() / 8 + 1);
    if (!o.empty())
        memcpy(g_base_offsets.data(), o.data(), o.size());
    g_base_bytes = strtoull(argv[4], nullptr, 10);
    const uint64_t align = strtoull(argv[5], nullptr, 10);
    Answer whole, bare;
    int err = lay(a, a.size(), b, b.size(), align, true, &whole);
    if (err)
    {
        printf("FAIL the valid blobs: errno %d\n", err);
        return 1;
    }
    printf("offsets");
    for (const uint64_t x : whole.offsets)
        printf(" %llu", (unsigned long long)x);
    printf("\ntotal %llu\nkept %u\n", (unsigned long long)whole.total, whole.kept);
    err = lay(a, a.size(), b, b.size(), align, false, &bare);
    if (err || bare.total != whole.total || bare.kept != whole.kept || bare.count != whole.count)
    {
        printf("FAIL without an offsets array: errno %d\n", err);
        return 1;
    }
    unsigned long long cases = 2;
    for (int side = 0; side < 2; ++side)
        for (size_t n = 0; n < (side ? b.size() : a.size()); ++n, ++cases)
        {
            Answer d;
            err = side ? lay(a, a.size(), b, n, align, true, &d) : lay(a, n, b, b.size(), align, true, &d);
            if (err != EBADF)
            {
                printf("FAIL prefix %zu of %s: errno %d, expected %d\n", n, side ? "the target" : "the base", err, EBADF);
                return 1;
            }
        }
    uint32_t count = 0;
    const int refusals[] = {
        restore_layout::in_place(nullptr, a.size(), g_base_offsets.data(), g_base_bytes, b.data(), b.size(), align, nullptr, &count, nullptr, nullptr),
        restore_layout::in_place(a.data(), a.size(), g_base_offsets.data(), g_base_bytes, nullptr, b.size(), align, nullptr, &count, nullptr, nullptr),
        restore_layout::in_place(a.data(), a.size(), nullptr, g_base_bytes, b.data(), b.size(), align, nullptr, &count, nullptr, nullptr),
        restore_layout::in_place(a.data(), a.size(), g_base_offsets.data(), g_base_bytes, b.data(), b.size(), 0, nullptr, &count, nullptr, nullptr),
        align > 1 ? restore_layout::in_place(a.data(), a.size(), g_base_offsets.data(), g_base_bytes, b.data(), b.size(), align + 1, nullptr, &count,
                                             nullptr, nullptr)
                  : EINVAL};
    for (const int r : refusals)
    {
        if (r != EINVAL)
        {
            printf("FAIL a refusal: errno %d, expected %d\n", r, EINVAL);
            return 1;
        }
        ++cases;
    }
    printf("ok %llu\n", cases);
    return 0;
}
