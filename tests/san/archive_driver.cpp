// archive_driver.cpp -- stand-alone driver of longtail_amd/csrc/archive_layout.h for tests/test_archive_san.py: built with
// -fsanitize=address,undefined and run as a program.  It includes the layout header and nothing else of the library.
//   archive_driver SI VI TABLES
// SI / VI hold VALID serialized indexes, TABLES u64 offsets[nb] followed by u32 sizes[nb].  Every buffer the header sees is a heap copy of
// exactly the bytes offered, placed at an ODD address (so that a load or store through a typed pointer is UBSan's to report, and a read
// past the bytes ASan's).  The driver
//   writes the index (too small a capacity first: ENOMEM, nothing written) and prints it in hex                       -> "index <hex>"
//   opens it with the body size known and unknown and prints what it read                              -> "open <nb> <body> <offsets> <sizes>"
//   offers every proper prefix, the index with a byte appended, and every 32-bit word of the head and of both count pairs set to
//   0xFFFFFFFF, 0x20000000, 0x40000000, 0x80000000, 0xAAAAAAAB (products that wrap 32 bits)                            -> EBADF
//   sets every block's offset in turn so that offset + size wraps 2^64, with and without a known body                  -> EBADF
//   merges a list of ranges at three gaps                                                               -> "ranges <gap>: <first>+<bytes> ..."
// and prints "ok <cases>"; the first wrong answer is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../longtail_amd/csrc/archive_layout.h"

// a heap copy of n bytes that starts at an odd address and ends where its allocation ends
struct Odd
{
    uint8_t* base;
    uint8_t* p;
    Odd(const uint8_t* src, size_t n) : base((uint8_t*)malloc(n + 1)), p(base + 1)
    {
        if (n)
            memcpy(p, src, n);
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

static int open_at_odd(const std::vector<uint8_t>& index, size_t size, uint64_t body, archive_layout::Archive* out = nullptr)
{
    Odd copy(index.data(), size);
    archive_layout::Archive a;
    const int err = archive_layout::open(copy.p, size, body, &a);
    if (!err && out)
        *out = a;
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
    if (argc != 4)
        return 2;
    const std::vector<uint8_t> si = slurp(argv[1]), vi = slurp(argv[2]), tables = slurp(argv[3]);
    const size_t nb = tables.size() / 12;
    Odd osi(si.data(), si.size()), ovi(vi.data(), vi.size()), otab(tables.data(), tables.size());
    // (the tables go through the typed interface the C entry points have: those two arrays are the caller's, aligned)
    std::vector<uint64_t> offsets(nb);
    std::vector<uint32_t> sizes(nb);
    if (nb)
    {
        memcpy(offsets.data(), otab.p, nb * 8);
        memcpy(sizes.data(), otab.p + nb * 8, nb * 4);
    }
    uint64_t cases = 0, bytes = 0;
    int bad = expect(archive_layout::index_size(osi.p, si.size(), ovi.p, vi.size(), &bytes), 0, "index_size", 0, 0);
    if (bad)
        return 1;
    std::vector<uint8_t> index(bytes, 0xEE);
    {
        Odd out(index.data(), bytes);
        bad = expect(archive_layout::write_index(osi.p, si.size(), ovi.p, vi.size(), offsets.data(), sizes.data(), out.p, bytes - 1), ENOMEM,
                     "write_index below the size", bytes, 0);
        for (uint64_t i = 0; i < bytes && !bad; ++i)
            bad = expect(out.p[i], 0xEE, "a refused write_index wrote", i, 0);
        if (!bad)
            bad = expect(archive_layout::write_index(osi.p, si.size(), ovi.p, vi.size(), offsets.data(), sizes.data(), out.p, bytes), 0,
                         "write_index", bytes, 0);
        memcpy(index.data(), out.p, bytes);
    }
    if (bad)
        return 1;
    printf("index ");
    for (const uint8_t b : index)
        printf("%02x", b);
    printf("\n");
    uint64_t end = 0;
    for (size_t b = 0; b < nb; ++b)
        end = std::max(end, offsets[b] + sizes[b]);
    for (const uint64_t body : {end, archive_layout::BODY_UNKNOWN})
    {
        archive_layout::Archive a;
        bad = bad || expect(open_at_odd(index, index.size(), body, &a), 0, "open", body, 0);
        if (bad)
            return 1;
        printf("open %zu %llu", a.offsets.size(), (unsigned long long)a.body_bytes);
        for (const uint64_t o : a.offsets)
            printf(" %llu", (unsigned long long)o);
        for (const uint32_t s : a.sizes)
            printf(" %u", s);
        printf("\n");
        ++cases;
    }
    if (nb)
        bad = expect(open_at_odd(index, index.size(), end - 1, nullptr), EBADF, "a body one byte short", end, 0), ++cases;
    for (size_t n = 0; n < index.size() && !bad; ++n, ++cases)
        bad = expect(open_at_odd(index, n, end), EBADF, "prefix", n, 0);
    if (!bad)
    {
        std::vector<uint8_t> x = index;
        x.push_back(0);
        bad = expect(open_at_odd(x, x.size(), end), EBADF, "over-long", x.size(), 0), ++cases;
    }
    // the words that place something: version, stored size, the StoreIndex's version / hash identifier / counts, the VersionIndex's head
    const size_t vi_at = 8 + archive_layout::store_index_bytes(nb, archive_layout::get32(index.data() + 20)) + 12 * nb;
    std::vector<size_t> words = {0, 4, 8, 12, 16, 20};
    for (const size_t w : {0, 1, 3, 4, 5}) // (word 2 is the target chunk size: any value below 2^31 is one)
        words.push_back(vi_at + 4 * w);
    static const uint32_t big[] = {0xFFFFFFFFu, 0x20000000u, 0x40000000u, 0x80000000u, 0xAAAAAAABu};
    for (const uint32_t v : big)
        for (size_t k = 0; k < words.size() && !bad; ++k, ++cases)
        {
            std::vector<uint8_t> x = index;
            memcpy(x.data() + words[k], &v, 4);
            bad = expect(open_at_odd(x, x.size(), end), EBADF, "head word", words[k], v);
        }
    for (size_t b = 0; b < nb && !bad; ++b)
        for (const uint64_t body : {end, archive_layout::BODY_UNKNOWN})
        {
            std::vector<uint8_t> x = index;
            const uint64_t off = ~0ull - sizes[b] + 1u; // offset + size == 2^64
            memcpy(x.data() + 8 + archive_layout::store_index_bytes(nb, archive_layout::get32(index.data() + 20)) + 8 * b, &off, 8);
            bad = bad || expect(open_at_odd(x, x.size(), body), EBADF, "offset + size wraps", b, body);
            ++cases;
        }
    if (bad)
        return 1;
    for (const uint64_t gap : {0ull, 9ull, ~0ull})
    {
        std::vector<std::pair<uint64_t, uint64_t>> r = {{100, 10}, {0, 10}, {10, 5}, {120, 1}, {105, 30}, {~0ull - 4, 4}, {200, 0}};
        archive_layout::merge_ranges(&r, gap);
        printf("ranges %llu:", (unsigned long long)gap);
        for (const auto& x : r)
            printf(" %llu+%llu", (unsigned long long)x.first, (unsigned long long)x.second);
        printf("\n");
        ++cases;
    }
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
