// A stand-alone program for tests/test_block_cache_san.py: it includes longtail_amd/csrc/block_cache.h alone, replays a script of
// operations on one block_cache::Table and prints the table's state after each, for the test to compare with its Python model.
// Built with -fsanitize=address,undefined and run as a program.
//   usage: block_cache_driver <script> <slots> <slot bytes>
//   script lines:  attach <id> <hash> <chunks> <raw> <digest> <need verified>   lookup + matches + pin -> the slot or -1
//                  reserve <id> <hash> <chunks> <raw> <digest>                   -> the slot or -1
//                  commit <slot> <verified> | abort <slot> <bad> | unpin <slot> | clear   -> 1 or 0
//                  digest <n> <hash> <size> ...                                  -> prints the table digest alone
#include "../../longtail_amd/csrc/block_cache.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace block_cache;

static void print_state(const Table& t, long long result)
{
    printf("%lld |", result);
    for (uint32_t i = 0; i < t.slot_count(); ++i)
    {
        const Slot& s = t.slot(i);
        if (s.state == FREE)
            printf(" %u:F", i);
        else
            printf(" %u:%c:%u/%" PRIu64 ":%u/%u/%" PRIu64 ":%u:%d", i, s.state == RESERVED ? 'R' : 'V', s.key.hash_identifier, s.key.block_hash,
                   s.meta.chunks, s.meta.raw, s.meta.digest, s.pins, s.verified ? 1 : 0);
    }
    printf(" | lru");
    for (const uint32_t i : t.lru_order())
        printf(" %u", i);
    if (t.lru_order().empty())
        printf(" ");
    const Counts& n = t.counts();
    printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", n.hits, n.inserted, n.evicted, n.bypassed, n.dropped);
}

int main(int argc, char** argv)
{
    if (argc != 4)
        return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f)
        return 2;
    Table t((uint32_t)strtoul(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    char op[16];
    uint64_t lines = 0;
    while (fscanf(f, "%15s", op) == 1)
    {
        long long result = 0;
        if (!strcmp(op, "attach") || !strcmp(op, "reserve"))
        {
            Key k;
            Meta m;
            unsigned need = 0;
            if (fscanf(f, "%u %" SCNu64 " %u %u %" SCNu64, &k.hash_identifier, &k.block_hash, &m.chunks, &m.raw, &m.digest) != 5)
                return 3;
            if (op[0] == 'a')
            {
                if (fscanf(f, "%u", &need) != 1)
                    return 3;
                const uint32_t s = t.lookup(k);
                result = s != NO_SLOT && t.matches(s, m, need != 0) && t.pin(s) ? (long long)s : -1;
            }
            else
            {
                const uint32_t s = t.reserve(k, m);
                result = s == NO_SLOT ? -1 : (long long)s;
            }
        }
        else if (!strcmp(op, "commit") || !strcmp(op, "abort"))
        {
            unsigned s = 0, flag = 0;
            if (fscanf(f, "%u %u", &s, &flag) != 2)
                return 3;
            result = op[0] == 'c' ? t.commit(s, flag != 0) : t.abort(s, flag != 0);
        }
        else if (!strcmp(op, "unpin"))
        {
            unsigned s = 0;
            if (fscanf(f, "%u", &s) != 1)
                return 3;
            result = t.unpin(s);
        }
        else if (!strcmp(op, "clear"))
            result = t.clear();
        else if (!strcmp(op, "digest"))
        {
            unsigned n = 0;
            if (fscanf(f, "%u", &n) != 1)
                return 3;
            std::vector<uint64_t> h(n);
            std::vector<uint32_t> z(n);
            for (unsigned j = 0; j < n; ++j)
                if (fscanf(f, "%" SCNu64 " %u", &h[j], &z[j]) != 2)
                    return 3;
            printf("digest %" PRIu64 "\n", table_digest(h.data(), z.data(), n));
            ++lines;
            continue;
        }
        else
            return 4;
        print_state(t, result);
        ++lines;
    }
    fclose(f);
    printf("ok %" PRIu64 "\n", lines);
    return 0;
}
