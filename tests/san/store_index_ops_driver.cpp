// store_index_ops_driver.cpp -- stand-alone driver of longtail_amd/csrc/store_index_ops.h for tests/test_store_index_ops_san.py: built
// with -fsanitize=address,undefined and run as a program.  It includes the header and nothing else of the library.
//   store_index_ops_driver LOCAL REMOTE KEEP VI
// LOCAL / REMOTE hold VALID serialized StoreIndexes, KEEP u64 block hashes, VI a valid serialized VersionIndex.  Every blob the header
// sees, and every output it writes, is a heap buffer of exactly the bytes offered that starts at an ODD address (so that a load or store
// through a typed pointer is UBSan's to report, and an access past the bytes ASan's).  The driver
//   prunes LOCAL by KEEP, merges LOCAL with REMOTE and REMOTE with LOCAL -- each first with one byte too few (ENOMEM, the size set,
//   nothing written) and with a null output, then for real                           -> "prune <hex>", "merge <hex>", "merge_rev <hex>"
//   (a merge the header refuses prints "merge errno <n>" instead)
//   lists VI's chunk hashes: the count alone, one entry too few (ENOMEM), all         -> "hashes <n> <h> ..."
//   offers every proper prefix of LOCAL to prune and to both sides of merge, and every proper prefix of VI           -> EBADF
//   sets every 32-bit word of LOCAL's head to 0xFFFFFFFF, 0x20000000, 0x40000000, 0x80000000, 0xAAAAAAAB             -> EBADF
//   points the first block's chunk run just past the chunk list                                                      -> EBADF
// and prints "ok <cases>"; the first wrong answer is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../longtail_amd/csrc/store_index_ops.h"

// a heap buffer of n bytes that starts at an odd address and ends where its allocation ends
struct Odd
{
    uint8_t* base;
    uint8_t* p;
    Odd(const uint8_t* src, size_t n) : base((uint8_t*)malloc(n + 1)), p(base + 1)
    {
        if (n && src)
            memcpy(p, src, n);
        else if (n)
            memset(p, 0xEE, n);
    }
    ~Odd() { free(base); }
};

static std::vector<uint8_t> slurp(const char* path)
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

static int expect(int got, int want, const char* what, uint64_t a, uint64_t b)
{
    if (got == want)
        return 0;
    printf("FAIL %s (%llu, %llu): %d, expected %d\n", what, (unsigned long long)a, (unsigned long long)b, got, want);
    return 1;
}

typedef std::vector<uint8_t> Blob;

// op(out, capacity, &size) three ways: a null output, one byte too few, the size asked for.  Prints "<name> <hex>" or "<name> errno <n>".
template <class Op> static int three_ways(const char* name, Op op, uint64_t* cases)
{
    size_t size = 0xEEEE;
    int err = op(nullptr, 0, &size);
    if (err != ENOMEM)
    {
        printf("%s errno %d\n", name, err);
        ++*cases;
        return 0;
    }
    const size_t need = size;
    int bad = 0;
    {
        Odd out(nullptr, need);
        size = 0xEEEE;
        bad = expect(op(out.p, need - 1, &size), ENOMEM, name, need, 0) || expect(size == need, 1, "the size of a refused call", size, need);
        for (size_t i = 0; i + 1 < need && !bad; ++i)
            bad = expect(out.p[i], 0xEE, "a refused call wrote", i, 0);
    }
    if (bad)
        return 1;
    Odd out(nullptr, need);
    size = 0;
    if (expect(op(out.p, need, &size), 0, name, need, 0) || expect(size == need, 1, "the size", size, need))
        return 1;
    printf("%s ", name);
    for (size_t i = 0; i < need; ++i)
        printf("%02x", out.p[i]);
    printf("\n");
    *cases += 3;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 5)
        return 2;
    const Blob local = slurp(argv[1]), remote = slurp(argv[2]), keep_bytes = slurp(argv[3]), vi = slurp(argv[4]);
    std::vector<uint64_t> keep(keep_bytes.size() / 8); // (the keep list is the caller's typed array)
    if (!keep.empty())
        memcpy(keep.data(), keep_bytes.data(), keep.size() * 8);
    Odd ol(local.data(), local.size()), orr(remote.data(), remote.size()), ov(vi.data(), vi.size());
    uint64_t cases = 0;
    namespace ops = store_index_ops;
    if (three_ways("prune", [&](void* o, size_t c, size_t* s) { return ops::prune(ol.p, local.size(), (uint32_t)keep.size(), keep.data(), o, c, s); }, &cases) ||
        three_ways("merge", [&](void* o, size_t c, size_t* s) { return ops::merge(ol.p, local.size(), orr.p, remote.size(), o, c, s); }, &cases) ||
        three_ways("merge_rev", [&](void* o, size_t c, size_t* s) { return ops::merge(orr.p, remote.size(), ol.p, local.size(), o, c, s); }, &cases))
        return 1;
    // the chunk hashes of VI
    uint64_t count = 0xEEEE;
    const int alone = ops::version_chunk_hashes(ov.p, vi.size(), nullptr, 0, &count);
    int bad = expect(alone, count ? ENOMEM : 0, "the count alone", count, 0);
    std::vector<uint64_t> hashes(count + 1, 0xEEEEEEEEEEEEEEEEull);
    if (!bad && count)
    {
        uint64_t again = 0;
        bad = expect(ops::version_chunk_hashes(ov.p, vi.size(), hashes.data(), count - 1, &again), ENOMEM, "one entry too few", count, again) ||
              expect(again == count && hashes[0] == 0xEEEEEEEEEEEEEEEEull, 1, "a refused listing", again, hashes[0]);
    }
    bad = bad || expect(ops::version_chunk_hashes(ov.p, vi.size(), hashes.data(), count, &count), 0, "the listing", count, 0) ||
          expect(hashes[count] == 0xEEEEEEEEEEEEEEEEull, 1, "the entry behind the listing", count, 0);
    if (bad)
        return 1;
    printf("hashes %llu", (unsigned long long)count);
    for (uint64_t i = 0; i < count; ++i)
        printf(" %llu", (unsigned long long)hashes[i]);
    printf("\n");
    cases += 3;
    // prefixes
    size_t size = 0;
    for (size_t n = 0; n < local.size() && !bad; ++n, ++cases)
    {
        Odd cut(local.data(), n);
        bad = expect(ops::prune(cut.p, n, (uint32_t)keep.size(), keep.data(), nullptr, 0, &size), EBADF, "prune of a prefix", n, 0) ||
              expect(ops::merge(cut.p, n, orr.p, remote.size(), nullptr, 0, &size), EBADF, "merge, a prefix as local", n, 0) ||
              expect(ops::merge(orr.p, remote.size(), cut.p, n, nullptr, 0, &size), EBADF, "merge, a prefix as remote", n, 0);
    }
    for (size_t n = 0; n < vi.size() && !bad; ++n, ++cases)
    {
        Odd cut(vi.data(), n);
        bad = expect(ops::version_chunk_hashes(cut.p, n, nullptr, 0, &count), EBADF, "the hashes of a prefix", n, 0);
    }
    // head words that wrap 32-bit products
    static const uint32_t big[] = {0xFFFFFFFFu, 0x20000000u, 0x40000000u, 0x80000000u, 0xAAAAAAABu};
    for (const uint32_t v : big)
        for (size_t w = 0; w < 4 && !bad; ++w, ++cases)
        {
            Blob x = local;
            memcpy(x.data() + 4 * w, &v, 4);
            Odd o(x.data(), x.size());
            bad = expect(ops::prune(o.p, x.size(), 0, nullptr, nullptr, 0, &size), EBADF, "head word", w, v) ||
                  expect(ops::merge(orr.p, remote.size(), o.p, x.size(), nullptr, 0, &size), EBADF, "head word, remote", w, v);
        }
    uint32_t nb, m;
    memcpy(&nb, local.data() + 8, 4);
    memcpy(&m, local.data() + 12, 4);
    if (nb && !bad)
    {
        Blob x = local;
        uint32_t count0;
        memcpy(&count0, x.data() + 16 + 8 * (size_t)nb + 8 * (size_t)m + 4 * (size_t)nb, 4);
        const uint32_t first = m - count0 + 1u; // the run ends one chunk behind the list
        memcpy(x.data() + 16 + 8 * (size_t)nb + 8 * (size_t)m, &first, 4);
        Odd o(x.data(), x.size());
        bad = expect(ops::prune(o.p, x.size(), 0, nullptr, nullptr, 0, &size), EBADF, "a chunk run past the list", first, count0);
        ++cases;
    }
    if (bad)
        return 1;
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
