// restore_call_driver.cpp -- stand-alone driver of longtail_amd/csrc/restore_call.h for tests/test_restore_call_san.py: built with
// -fsanitize=address,undefined and run as a program.  It includes the header and nothing else of the library.
//   restore_call_driver SCRIPT
// SCRIPT is text, one step per line; the driver prints one line per step that has an answer.
//   block HASH TAG CHUNKS RAW ENTRIES FED   one more block of the session's StoreIndex (ENTRIES: its entries in the plan; FED: cache-fed)
//   entries B N                             block B of the definitions gets N entries
//   reset                                   the state is built anew from the definitions: nothing delivered
//   stamp N                                 the call counter of the duplicate stamps becomes N
//   call FILE COUNT ANY SCRATCH SCRATCH_BYTES OUT IN_PLACE_BUF   a blocks call by hashes.  FILE holds u64 hashes[COUNT], u64 offsets[COUNT],
//                                           u32 sizes[COUNT]; the three pointers are numbers (0: null) and are never followed
//   calli ...                               the same call by block indices, resolved before (a hash the state lacks: the call is not made)
//   archive BODY then COUNT lines  HASH OFFSET SIZE   the archive of the picks that follow
//   pick FIRST BYTES                        the pick of body bytes [FIRST, FIRST + BYTES)
// Every array of a call is a heap copy of exactly its bytes at an ODD address that ends where its allocation ends: a load through a typed
// pointer is UBSan's to report, a read past the bytes ASan's.  Before a call the whole state is copied; a refused call must leave it as it
// was ("STATE CHANGED" and exit status 1 otherwise).  Answers:
//   refused ERRNO WHY
//   ok blocks=.. scratch=N any=0|1 groups=..|..|.. counters=needed,needed_delivered,delivered_all,unneeded bound=N
//        (groups: positions in the call; bound: restore_call::scratch_bound of the same hashes, asked before the call)
//   pick blocks=.. offsets=.. sizes=.. scratch=N next=N
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>

#include "../../longtail_amd/csrc/restore_call.h"

using restore_call::Blocks;

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

struct Def
{
    uint64_t hash;
    uint32_t tag, chunks, raw, entries, fed;
};

static Blocks build(const std::vector<Def>& defs)
{
    Blocks s;
    for (const Def& d : defs)
        s.st.bhash.push_back(d.hash), s.st.btag.push_back(d.tag), s.st.bcnt.push_back(d.chunks), s.st.braw.push_back(d.raw);
    s.init();
    for (size_t b = 0; b < defs.size(); ++b)
    {
        s.firsts[b + 1] = s.firsts[b] + defs[b].entries;
        s.fed[b] = (uint8_t)defs[b].fed;
    }
    for (uint32_t b = 0; b < defs.size(); ++b)
        s.needed += s.is_needed(b);
    return s;
}

// everything of the state but the stamps, which no answer depends on
static bool same(const Blocks& a, const Blocks& b)
{
    return a.st.bhash == b.st.bhash && a.st.btag == b.st.btag && a.st.bcnt == b.st.bcnt && a.st.braw == b.st.braw && a.firsts == b.firsts &&
           a.fed == b.fed && a.delivered == b.delivered && a.block_of_hash == b.block_of_hash && a.needed == b.needed &&
           a.needed_delivered == b.needed_delivered && a.delivered_all == b.delivered_all && a.unneeded == b.unneeded;
}

template <class V> static std::string list(const V& v)
{
    std::string out;
    for (const auto x : v)
        out += (out.empty() ? "" : ",") + std::to_string((unsigned long long)x);
    return out;
}

int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    std::ifstream script(argv[1]);
    if (!script)
        return 2;
    std::vector<Def> defs;
    Blocks s;
    restore_call::Call c;
    archive_layout::Archive a;
    std::string line, op;
    while (std::getline(script, line))
    {
        std::istringstream in(line);
        if (!(in >> op))
            continue;
        if (op == "block")
        {
            Def d;
            in >> d.hash >> d.tag >> d.chunks >> d.raw >> d.entries >> d.fed;
            defs.push_back(d);
        }
        else if (op == "entries")
        {
            size_t b;
            in >> b;
            in >> defs.at(b).entries;
        }
        else if (op == "reset")
            s = build(defs);
        else if (op == "stamp")
            in >> s.stamps.call;
        else if (op == "call" || op == "calli")
        {
            std::string file;
            uint32_t count, any;
            uint64_t scratch, scratch_bytes, out, in_place;
            in >> file >> count >> any >> scratch >> scratch_bytes >> out >> in_place;
            std::ifstream f(file, std::ios::binary);
            std::vector<uint8_t> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            if (!in || raw.size() != (size_t)count * 20u)
                return 2;
            const Odd hashes(raw.data(), count * 8u), offsets(raw.data() + count * 8u, count * 8u), sizes(raw.data() + count * 16u, count * 4u);
            std::vector<uint32_t> indices;
            for (uint32_t i = 0; i < count && op == "calli"; ++i)
                indices.push_back(s.find(restore_call::get64(hashes.p + 8u * i)));
            if (std::find(indices.begin(), indices.end(), restore_call::NONE) != indices.end())
                return 2;
            const Blocks before = s;
            const uint64_t bound = restore_call::scratch_bound(s, count, hashes.p);
            const restore_call::Where w{(const void*)(uintptr_t)scratch, (const void*)(uintptr_t)out, (const void*)(uintptr_t)in_place, scratch_bytes,
                                        any != 0};
            const int refused = restore_call::resolve(s, count, op == "call" ? hashes.p : nullptr, indices.data(), offsets.p, w, &c);
            if (refused)
            {
                if (!same(s, before))
                    return printf("STATE CHANGED by a refused call\n"), 1;
                printf("refused %d %s\n", refused, c.why);
                continue;
            }
            restore_call::commit(&s, &c, sizes.p);
            printf("ok blocks=%s scratch=%llu any=%d groups=%s|%s|%s counters=%llu,%llu,%llu,%llu bound=%llu\n", list(c.blocks).c_str(),
                   (unsigned long long)c.scratch, (int)c.any_needed, list(c.group[0]).c_str(), list(c.group[1]).c_str(), list(c.group[2]).c_str(),
                   (unsigned long long)s.needed, (unsigned long long)s.needed_delivered, (unsigned long long)s.delivered_all,
                   (unsigned long long)s.unneeded, (unsigned long long)bound);
        }
        else if (op == "archive")
        {
            size_t count;
            in >> a.body_bytes >> count;
            a.bhash.resize(count), a.offsets.resize(count), a.sizes.resize(count);
            for (size_t i = 0; i < count; ++i)
                script >> a.bhash[i] >> a.offsets[i] >> a.sizes[i];
        }
        else if (op == "pick")
        {
            uint64_t first, bytes;
            in >> first >> bytes;
            const Blocks before = s;
            restore_call::Pick p;
            restore_call::pick(s, a, first, bytes, &p);
            if (!same(s, before))
                return printf("STATE CHANGED by a pick\n"), 1;
            printf("pick blocks=%s offsets=%s sizes=%s scratch=%llu next=%llu\n", list(p.blocks).c_str(), list(p.offsets).c_str(),
                   list(p.sizes).c_str(), (unsigned long long)p.scratch, (unsigned long long)p.next_byte);
        }
        else
            return 2;
        if (!in && op != "archive")
            return 2;
    }
    printf("done\n");
    return 0;
}
