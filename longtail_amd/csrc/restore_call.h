// restore_call.h -- the host side of a restore session's blocks call, on the host and without a line of HIP: which blocks a call names,
// whether it is refused, what it costs in scratch, what it changes.  Kept apart from the device code so that a sanitizer can reach it.
//   Blocks         the per-block host state a call reads and changes; slot_bytes(b) is the one place that says what a block costs in
//                  scratch, scratch_bound sums it over hashes (an unknown hash, an unneeded or a cache-fed block costs nothing)
//   resolve        a call's hashes (or block indices already known) -> its block indices, scratch sum, "any needed", or its refusal
//   commit         an accepted call: delivered, the counters, its needed blocks in three groups (not decoded, LZ4, zstd) in call order
//   pick           an archive's needed, outstanding blocks that lie wholly inside a window of its body, in the archive's order
// The caller's hash, offset and size arrays are read with memcpy: no alignment is asked of them.  May throw std::bad_alloc.
// Included by restore.hip and by the stand-alone driver tests/san/restore_call_driver.cpp.
#pragma once
#include "archive_layout.h"
#include "restore_plan.h"
#include "store_layout.h"

#include <unordered_map>

namespace restore_call
{

using archive_layout::get64;
using restore_plan::NONE;

inline uint64_t round64(uint64_t x) { return (x + 63u) & ~(uint64_t)63u; }

// "twice in this call" by generation: a block is marked when its stamp is the current call's number, so nothing is taken back
struct Stamps
{
    std::vector<uint32_t> of;
    uint32_t call = 0;
    void next() // a new call: no block is marked.  A counter that wraps would meet the stamps of 2^32 calls ago: the table is cleared
    {
        if (++call == 0u)
            std::fill(of.begin(), of.end(), 0u), call = 1u;
    }
    bool marked(uint32_t b) const { return of[b] == call; }
    void mark(uint32_t b) { of[b] = call; }
};

struct Blocks
{
    restore_plan::StoreTables st;                         // the StoreIndex on the host (cblock and coff are given up once they are uploaded)
    std::vector<uint32_t> firsts;                         // block_count + 1: every block's first entry in the plan
    std::vector<uint8_t> fed, delivered;                  // fed: the block comes from a cache and is no longer needed
    std::unordered_map<uint64_t, uint32_t> block_of_hash; // (of blocks that share a hash, the first)
    uint64_t needed = 0, needed_delivered = 0, delivered_all = 0, unneeded = 0;
    mutable Stamps stamps; // the one mutable member: a query marks the blocks it has seen, and no answer depends on an earlier call's marks

    void init() // st is set: everything else for its blocks, nothing delivered, no entries yet
    {
        const size_t nb = st.bhash.size();
        for (size_t b = 0; b < nb; ++b)
            block_of_hash.emplace(st.bhash[b], (uint32_t)b);
        delivered.assign(nb, 0), fed.assign(nb, 0), firsts.assign(nb + 1, 0u), stamps.of.assign(nb, 0u);
    }
    uint32_t find(uint64_t hash) const
    {
        const auto it = block_of_hash.find(hash);
        return it == block_of_hash.end() ? NONE : it->second;
    }
    bool is_needed(uint32_t b) const { return firsts[b + 1] != firsts[b] && !fed[b]; }
    // the scratch a delivered block is decoded into: a needed block that carries a tag takes its raw size in 64-byte units
    uint64_t slot_bytes(uint32_t b) const { return is_needed(b) && st.btag[b] != 0u ? round64(st.braw[b]) : 0u; }
};

inline uint64_t scratch_bound(const Blocks& s, uint32_t count, const void* hashes)
{
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < count; ++i)
        if (const uint32_t b = s.find(get64((const uint8_t*)hashes + 8u * i)); b != NONE)
            bytes += s.slot_bytes(b);
    return bytes;
}

// where a call's images lie and where its bytes go
struct Where
{
    const void *scratch, *out, *in_place_buf; // in_place_buf: the buffer an in-place carry was given, or null
    uint64_t scratch_bytes;
    bool any_position; // the images lie at any byte positions: no offset is refused
};

// one blocks call, kept by the session for its capacity
struct Call
{
    std::vector<uint32_t> blocks;   // its block indices, in call order
    std::vector<uint32_t> group[3]; // commit: the POSITIONS in the call of its needed blocks -- not decoded, LZ4, zstd
    uint64_t scratch = 0;           // slot_bytes summed
    bool any_needed = false;
    const char* why = ""; // of a refusal
};

// The blocks of a call: `hashes`, or (hashes == null) the `indices` of blocks that were resolved before; `offsets`: the images' (not read
// with any_position).  0, or the refusal -- the first position that refuses decides, in the order ENOENT, EEXIST, EINVAL (alignment),
// ENOTSUP; a call whose every position passes is then held against `w`.  Changes nothing of the state.
inline int resolve(const Blocks& s, uint32_t count, const void* hashes, const uint32_t* indices, const void* offsets, const Where& w, Call* c)
{
    c->blocks.clear(), c->scratch = 0, c->any_needed = false;
    s.stamps.next();
    for (uint32_t i = 0; i < count; ++i)
    {
        const uint32_t b = hashes ? s.find(get64((const uint8_t*)hashes + 8u * i)) : indices[i];
        if (b == NONE)
            return c->why = "a block hash the store index does not hold", ENOENT;
        if (s.delivered[b] || s.stamps.marked(b))
            return c->why = "a block was delivered before, or twice in this call", EEXIST;
        s.stamps.mark(b);
        c->blocks.push_back(b);
        if (!w.any_position && (get64((const uint8_t*)offsets + 8u * i) & 7u))
            return c->why = "image offsets must be 8-byte aligned", EINVAL;
        if (!s.is_needed(b))
            continue;
        c->any_needed = true;
        if (codec_of_tag(s.st.btag[b]) < 0)
            return c->why = "a needed block's tag names no codec of this library", ENOTSUP;
        c->scratch += s.slot_bytes(b);
    }
    if (c->scratch > w.scratch_bytes)
        return c->why = "scratch below lthip_restore_scratch_bound", ENOMEM;
    if ((c->scratch && !w.scratch) || (c->any_needed && !w.out))
        return c->why = "null scratch or output", EINVAL;
    if (c->any_needed && w.in_place_buf && w.out != w.in_place_buf)
        return c->why = "the base was carried in place: the output is that buffer", EINVAL;
    return 0;
}

// An accepted call is delivered.  sizes: the bytes of its images; an image no longer than its header has no payload to decode.
inline void commit(Blocks* s, Call* c, const void* sizes)
{
    for (auto& g : c->group)
        g.clear(), g.reserve(c->blocks.size()); // (what can throw comes before the first change)
    for (uint32_t i = 0; i < (uint32_t)c->blocks.size(); ++i)
    {
        const uint32_t b = c->blocks[i];
        s->delivered[b] = 1, ++s->delivered_all;
        ++(s->is_needed(b) ? s->needed_delivered : s->unneeded);
        if (!s->is_needed(b))
            continue;
        const int codec = codec_of_tag(s->st.btag[b]);
        const bool payload = (uint64_t)archive_layout::get32((const uint8_t*)sizes + 4u * i) > archive_layout::block_header_bytes(s->st.bcnt[b], s->st.btag[b]);
        c->group[codec == LTHIP_CODEC_NONE || !payload ? 0 : codec == LTHIP_CODEC_LZ4 ? 1 : 2].push_back(i);
    }
}

// Fed from an archive's body: the needed, not yet delivered blocks that lie wholly inside body bytes [first, first + bytes) (saturating
// at 2^64 - 1), in the archive's block order.  A block of the archive that the session does not hold is passed over, one the archive
// lists twice is picked once.
struct Pick
{
    std::vector<uint32_t> blocks, sizes;
    std::vector<uint64_t> offsets;          // relative to `first`
    uint64_t scratch = 0, next_byte = 0;    // next_byte: the lowest offset of an outstanding block outside the window, else the body's size
};
inline void pick(const Blocks& s, const archive_layout::Archive& a, uint64_t first, uint64_t bytes, Pick* p)
{
    const uint64_t end = first + bytes < first ? ~0ull : first + bytes;
    p->next_byte = a.body_bytes;
    s.stamps.next();
    for (size_t i = 0; i < a.bhash.size(); ++i)
    {
        const uint32_t b = s.find(a.bhash[i]);
        if (b == NONE || !s.is_needed(b) || s.delivered[b] || s.stamps.marked(b))
            continue;
        const uint64_t off = a.offsets[i], size = a.sizes[i];
        if (off < first || off + size > end) // (off + size does not wrap: archive_layout::open)
            p->next_byte = std::min(p->next_byte, off);
        else
        {
            s.stamps.mark(b), p->scratch += s.slot_bytes(b);
            p->blocks.push_back(b), p->offsets.push_back(off - first), p->sizes.push_back((uint32_t)size);
        }
    }
}

} // namespace restore_call
