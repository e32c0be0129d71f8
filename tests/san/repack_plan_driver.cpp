// repack_plan_driver.cpp -- stand-alone driver of longtail_amd/csrc/repack_plan.h (over restore_parse.h) for
// tests/test_repack_plan_san.py: built with -fsanitize=address,undefined and run as a program.  It includes the header and nothing else
// of the library.
//   repack_plan_driver NEW STORE KEPT
// NEW, STORE and KEPT hold VALID serialized StoreIndexes: a new index, a store's index and the index of the blocks kept of it.  Every
// blob is offered as a heap copy that starts at an ODD address and ends where its allocation ends (a read past it, or an aligned read of
// it, is the sanitizer's to report).  Printed, one per line:
//   block B first F raw R tag T stage S image I cap C dest D      per block of NEW (stage -1: a tag-0 block is not staged)
//   staging N / work N / moved N
//   kept 0 1 ...                                                   per block of STORE: KEPT names it
//   tags <hex>                                                     KEPT with the blocks' own tags, as bytes
//   refused A B C                                                  the refusals: a block of 4 GiB (EINVAL), blocks that do not list the
//                                                                  chunks in turn (EBADF), chunks no block lists (EBADF)
// and "ok" last; the first wrong answer is printed and the exit status is 1.  The codec bound is a model the test shares:
// 'lz42' raw + raw / 255 + 16, every other tag raw + raw / 256 + 64.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../longtail_amd/csrc/repack_plan.h"

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

// a heap copy at an odd address that ends where its allocation ends
struct OddCopy
{
    uint8_t* base;
    uint8_t* p;
    size_t n;
    explicit OddCopy(const std::vector<uint8_t>& v) : base((uint8_t*)malloc(v.size() + 1)), p(base + 1), n(v.size())
    {
        if (n)
            memcpy(p, v.data(), n);
    }
    ~OddCopy() { free(base); }
};

static uint64_t model_bound(uint32_t tag, uint32_t raw) { return tag == 0x6C7A3432u ? (uint64_t)raw + raw / 255u + 16u : (uint64_t)raw + raw / 256u + 64u; }

// a StoreIndex over hand-made arrays that parse_store_index would refuse: the arrays are the caller's
static std::vector<uint8_t> blob_of(const std::vector<uint32_t>& offs, const std::vector<uint32_t>& counts, const std::vector<uint32_t>& tags,
                                    const std::vector<uint32_t>& sizes)
{
    const uint32_t nb = (uint32_t)offs.size(), m = (uint32_t)sizes.size();
    std::vector<uint8_t> v(16 + 20u * nb + 12u * m, 0);
    const uint32_t head[4] = {restore_parse::STORE_INDEX_VERSION, 0x626c6b33u, nb, m};
    memcpy(v.data(), head, 16);
    uint8_t* w = v.data() + 16 + 8u * nb + 8u * m;
    memcpy(w, offs.data(), 4u * nb), memcpy(w + 4u * nb, counts.data(), 4u * nb), memcpy(w + 8u * nb, tags.data(), 4u * nb);
    memcpy(w + 12u * nb, sizes.data(), 4u * m);
    return v;
}
static restore_parse::StoreIndex view(const OddCopy& c)
{
    restore_parse::StoreIndex s;
    uint32_t head[4];
    memcpy(head, c.p, 16);
    s.hash_identifier = head[1], s.block_count = head[2], s.chunk_count = head[3];
    const uint64_t nb = head[2], m = head[3];
    s.block_hashes.p = c.p + 16;
    s.chunk_hashes.p = s.block_hashes.p + 8u * nb;
    s.block_chunk_offsets.p = s.chunk_hashes.p + 8u * m;
    s.block_chunk_counts.p = s.block_chunk_offsets.p + 4u * nb;
    s.block_tags.p = s.block_chunk_counts.p + 4u * nb;
    s.chunk_sizes.p = s.block_tags.p + 4u * nb;
    return s;
}
static int refusal(const std::vector<uint8_t>& blob)
{
    const OddCopy c(blob);
    repack_plan::Layout l;
    const char* why = "";
    return repack_plan::layout(view(c), model_bound, &l, &why);
}

int main(int argc, char** argv)
{
    if (argc != 4)
        return 2;
    const OddCopy fresh(read_file(argv[1])), store(read_file(argv[2])), kept(read_file(argv[3]));
    restore_parse::StoreIndex ni, si, ki;
    if (restore_parse::parse_store_index(fresh.p, fresh.n, &ni) || restore_parse::parse_store_index(store.p, store.n, &si) ||
        restore_parse::parse_store_index(kept.p, kept.n, &ki))
    {
        printf("FAIL a blob does not parse\n");
        return 1;
    }
    repack_plan::Layout l;
    const char* why = "";
    const int err = repack_plan::layout(ni, model_bound, &l, &why);
    if (err)
    {
        printf("FAIL layout: errno %d (%s)\n", err, why);
        return 1;
    }
    for (uint32_t b = 0; b < ni.block_count; ++b)
        printf("block %u first %u raw %u tag %u stage %lld image %llu cap %llu dest %llu\n", b, l.first[b], l.raw[b], l.tag[b],
               l.stage[b] == repack_plan::NOWHERE ? -1ll : (long long)l.stage[b], (unsigned long long)l.image[b], (unsigned long long)l.image_cap[b],
               (unsigned long long)l.dest[b]);
    printf("staging %llu\nwork %llu\nmoved %llu\n", (unsigned long long)l.staging_bytes, (unsigned long long)l.work_bytes,
           (unsigned long long)l.moved_bytes);
    std::vector<uint8_t> is_kept;
    repack_plan::block_lists(si, ki, &is_kept);
    printf("kept");
    for (const uint8_t k : is_kept)
        printf(" %u", k);
    printf("\ntags ");
    repack_plan::own_tags(si, ki, kept.p);
    for (size_t i = 0; i < kept.n; ++i)
        printf("%02x", kept.p[i]);
    const int a = refusal(blob_of({0}, {2}, {0}, {0xFFFFFFFFu, 1u}));
    const int b = refusal(blob_of({0, 2}, {1, 1}, {0, 0}, {5, 6, 7}));
    const int c = refusal(blob_of({0}, {1}, {7}, {5, 6}));
    printf("\nrefused %d %d %d\n", a, b, c);
    if (a != EINVAL || b != EBADF || c != EBADF)
    {
        printf("FAIL a refusal\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}
