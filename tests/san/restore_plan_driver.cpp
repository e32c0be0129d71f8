// restore_plan_driver.cpp -- stand-alone driver of longtail_amd/csrc/restore_plan.h (over restore_parse.h and restore_windows.h) for
// tests/test_restore_plan_san.py: built with -fsanitize=address,undefined and run as a program.  It includes the header and nothing
// else of the library.
//   restore_plan_driver store SI                    -> the tables of store_tables, one line each: "name v v v ..."
//   restore_plan_driver base VI OFFSETS BASE_BYTES  -> "max_chunk N", "hash ...", "size ...", "off ..."
//   restore_plan_driver whole VI OFFSETS            -> one line "asset offset length dst" per window
// SI / VI hold a VALID serialized index, OFFSETS one u64 per asset.  Every table is offered as a heap copy of exactly its bytes (a read
// past them is the sanitizer's to report).  A refusal prints "refused <errno> <why>" and is no failure of the driver: the exit status
// is 0 unless an index does not parse (2) or a refusal names no reason (1).
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../longtail_amd/csrc/restore_plan.h"

struct Blob
{
    uint8_t* p = nullptr;
    size_t n = 0;
    explicit Blob(const char* path)
    {
        std::vector<uint8_t> all;
        FILE* f = fopen(path, "rb");
        if (!f)
            exit(2);
        uint8_t buf[4096];
        for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;)
            all.insert(all.end(), buf, buf + k);
        fclose(f);
        n = all.size();
        p = (uint8_t*)malloc(n ? n : 1);
        if (n)
            memcpy(p, all.data(), n);
    }
    ~Blob() { free(p); }
};

template <class T> static void line(const char* name, const std::vector<T>& v)
{
    printf("%s", name);
    for (const T x : v)
        printf(" %llu", (unsigned long long)x);
    printf("\n");
}

static int refused(int err, const char* why)
{
    printf("refused %d %s\n", err, why ? why : "");
    return why && *why ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc < 3)
        return 2;
    const std::string mode = argv[1];
    const Blob index(argv[2]);
    const char* why = nullptr;
    if (mode == "store" && argc == 3)
    {
        restore_parse::StoreIndex si;
        if (restore_parse::parse_store_index(index.p, index.n, &si))
            return 2;
        restore_plan::StoreTables st;
        const int err = restore_plan::store_tables(si, &st, &why);
        if (err)
            return refused(err, why);
        printf("max_chunk %u\nblock_chunks %llu\n", st.max_chunk, (unsigned long long)st.block_chunks);
        line("chash", st.chash), line("csize", st.csize), line("cblock", st.cblock), line("coff", st.coff);
        line("bhash", st.bhash), line("bcoff", st.bcoff), line("bcnt", st.bcnt), line("btag", st.btag), line("braw", st.braw);
        line("bleaves", st.bleaves);
        return 0;
    }
    restore_parse::VersionIndex vi;
    if (restore_parse::parse_version_index(index.p, index.n, &vi) || argc < 4)
        return 2;
    const Blob offsets(argv[3]);
    if (offsets.n != (size_t)vi.asset_count * 8u)
        return 2;
    if (mode == "base" && argc == 5)
    {
        restore_plan::BaseTable bt;
        const int err = restore_plan::base_table(vi, (const uint64_t*)offsets.p, strtoull(argv[4], nullptr, 10), &bt, &why);
        if (err)
            return refused(err, why);
        printf("max_chunk %u\n", bt.max_chunk);
        line("hash", bt.hash), line("size", bt.size), line("off", bt.off);
        return 0;
    }
    if (mode == "whole" && argc == 4)
    {
        for (const restore_windows::Window& w : restore_plan::whole_asset_windows(vi, (const uint64_t*)offsets.p))
            printf("%u %llu %llu %llu\n", w.asset, (unsigned long long)w.offset, (unsigned long long)w.length, (unsigned long long)w.dst);
        return 0;
    }
    return 2;
}
