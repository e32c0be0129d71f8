// restore_windows_driver.cpp -- stand-alone driver of longtail_amd/csrc/restore_windows.h (over restore_parse.h) for
// tests/test_restore_windows_san.py: built with -fsanitize=address,undefined and run as a program.  It includes the header and nothing
// else of the library.
//   restore_windows_driver VI WINDOWS BAD OUT_BYTES [BIG_VI COUNT]
// VI holds a VALID serialized VersionIndex, WINDOWS and BAD hold lthip_restore_window records (32 bytes each): WINDOWS a valid set for an
// output of OUT_BYTES bytes, BAD windows that are each invalid on their own.  Every table is offered as a heap copy of exactly its
// bytes (a read past them is the sanitizer's to report):
//   VI whole with WINDOWS                  -> 0: "selected N", then one line "hash length skip clip dst" per occurrence
//   the asset sizes of VI                  -> 0: "sizes ..." and "target N"
//   each window of BAD alone, a null table -> EINVAL, nothing planned
//   every proper prefix of VI              -> EBADF from the parse and from asset_sizes
//   COUNT windows over all of asset 0 of BIG_VI -> EINVAL (too many occurrences), refused before anything of that size is allocated
// and prints "ok <cases>" last; the first wrong answer is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../longtail_amd/csrc/restore_windows.h"

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

// parse + expand over heap copies of exactly n bytes of the blob and exactly `count` windows
static int plan(const std::vector<uint8_t>& blob, size_t n, const restore_windows::Window* windows, uint64_t count, uint64_t out_bytes,
                restore_windows::Occurrences* out)
{
    uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
    if (n)
        memcpy(copy, blob.data(), n);
    restore_windows::Window* w = (restore_windows::Window*)malloc(count ? count * sizeof *w : 1);
    if (count && windows)
        memcpy(w, windows, count * sizeof *w);
    restore_parse::VersionIndex v;
    int err = restore_parse::parse_version_index(copy, n, &v);
    const char* why = nullptr;
    if (!err)
        err = restore_windows::expand(v, count, windows ? w : nullptr, out_bytes, out, &why);
    if (err && err != EBADF && (!why || !*why))
        err = -1; // a refusal names its reason
    free(w);
    free(copy);
    return err;
}

int main(int argc, char** argv)
{
    if (argc != 5 && argc != 7)
        return 2;
    const std::vector<uint8_t> vi = read_file(argv[1]), wf = read_file(argv[2]), bf = read_file(argv[3]);
    const uint64_t out_bytes = strtoull(argv[4], nullptr, 10);
    std::vector<restore_windows::Window> good(wf.size() / 32), bad(bf.size() / 32);
    if (!good.empty())
        memcpy(good.data(), wf.data(), good.size() * 32);
    if (!bad.empty())
        memcpy(bad.data(), bf.data(), bad.size() * 32);
    unsigned long long cases = 0;
    {
        restore_windows::Occurrences occ;
        const int err = plan(vi, vi.size(), good.data(), good.size(), out_bytes, &occ);
        if (err)
        {
            printf("FAIL the valid windows: errno %d\n", err);
            return 1;
        }
        printf("selected %llu\n", (unsigned long long)occ.assets_selected);
        for (size_t i = 0; i < occ.hash.size(); ++i)
            printf("%llu %u %u %u %llu\n", (unsigned long long)occ.hash[i], occ.len[i], occ.skip.empty() ? 0u : occ.skip[i],
                   occ.clip.empty() ? occ.len[i] : occ.clip[i], (unsigned long long)occ.dst[i]);
        ++cases;
    }
    {
        uint32_t assets = 0, target = 0;
        if (vi.size() >= 16)
            memcpy(&assets, vi.data() + 12, 4);
        uint64_t* sizes = (uint64_t*)malloc(assets ? assets * 8u : 1);
        uint32_t count = 0;
        const int err = restore_windows::asset_sizes(vi.data(), vi.size(), sizes, &count, &target);
        if (err || count != assets || restore_windows::asset_sizes(vi.data(), vi.size(), nullptr, nullptr, nullptr) ||
            restore_windows::asset_sizes(nullptr, vi.size(), sizes, &count, &target) != EINVAL)
        {
            printf("FAIL asset_sizes: errno %d\n", err);
            return 1;
        }
        printf("sizes");
        for (uint32_t a = 0; a < count; ++a)
            printf(" %llu", (unsigned long long)sizes[a]);
        printf("\ntarget %u\n", target);
        free(sizes);
        ++cases;
    }
    for (size_t i = 0; i <= bad.size(); ++i, ++cases)
    {
        restore_windows::Occurrences occ;
        const int err = i < bad.size() ? plan(vi, vi.size(), &bad[i], 1, out_bytes, &occ) : plan(vi, vi.size(), nullptr, 1, out_bytes, &occ);
        if (err != EINVAL || !occ.hash.empty())
        {
            printf("FAIL invalid window %zu: errno %d, expected %d\n", i, err, EINVAL);
            return 1;
        }
    }
    for (size_t n = 0; n < vi.size(); ++n, ++cases)
    {
        restore_windows::Occurrences occ;
        uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
        memcpy(copy, vi.data(), n);
        uint32_t count = 0;
        const int a = restore_windows::asset_sizes(copy, n, nullptr, &count, nullptr);
        free(copy);
        const int err = plan(vi, n, good.data(), good.size(), out_bytes, &occ);
        if (err != EBADF || a != EBADF)
        {
            printf("FAIL prefix %zu: errno %d / %d, expected %d\n", n, err, a, EBADF);
            return 1;
        }
    }
    if (argc == 7)
    {
        const std::vector<uint8_t> big = read_file(argv[5]);
        uint64_t size = 0;
        if (big.size() >= 24 + 24)
            memcpy(&size, big.data() + 24 + 16, 8); // asset 0's size: the version has one asset
        const std::vector<restore_windows::Window> many((size_t)strtoull(argv[6], nullptr, 10), restore_windows::Window{0u, 0u, 0u, size, 0u});
        restore_windows::Occurrences occ;
        const int err = plan(big, big.size(), many.data(), many.size(), size, &occ);
        if (err != EINVAL || occ.hash.capacity())
        {
            printf("FAIL too many occurrences: errno %d, expected %d\n", err, EINVAL);
            return 1;
        }
        ++cases;
    }
    printf("ok %llu\n", cases);
    return 0;
}
