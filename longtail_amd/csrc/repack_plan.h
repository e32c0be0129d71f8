// repack_plan.h -- the host arithmetic of a repack session (repack.hip), on the host and without a line of HIP, kept apart from the device
// code so that a sanitizer can reach it:
//   layout       the new index (what lthip_create_missing_content returned for the moved chunks) -> the caller's one work buffer: a
//                STAGING region, then the IMAGE region.  A tagged new block's chunks are staged back to back in the new index's chunk
//                order, block after block, so its raw payload is one byte range the codec reads where it lies.  A tag-0 new block's
//                chunks go straight to their final positions inside its image, behind where the BlockIndex will be written, and never
//                pass through staging.  Image offsets are 8-byte aligned; an image has room for lthip_stored_block_header_size(n) + the
//                codec's bound of its raw size, or lthip_block_index_size(n) + its raw size for tag 0.
//   block_lists  which blocks of the store stay (those the kept index names), which go, in StoreIndex order
//   own_tags     the kept index with every block's tag word set to the tag the store's own index records for that block
// The blobs are untrusted bytes of any alignment and are read through restore_parse.h.  May throw std::bad_alloc.
// Included by repack.hip and by the stand-alone driver tests/san/repack_plan_driver.cpp.
#pragma once
#include "restore_parse.h"

#include <unordered_map>
#include <vector>

namespace repack_plan
{

constexpr uint64_t NOWHERE = ~0ull; // a tag-0 block has no place in the staging region

inline uint64_t align8(uint64_t x) { return (x + 7u) & ~(uint64_t)7u; }
// the bytes in front of a block's payload: the BlockIndex (Longtail_GetBlockIndexDataSize), and for a tagged block the
// [raw][compressed] words -- lthip_block_index_size / lthip_stored_block_header_size
inline uint64_t header_bytes(uint32_t chunks, uint32_t tag) { return 20u + 12ull * chunks + (tag ? 8u : 0u); }

// the codec's bound of `raw` bytes for a block that carries `tag` (not asked for tag 0)
typedef uint64_t (*Bound)(uint32_t tag, uint32_t raw);

struct Layout
{
    std::vector<uint32_t> first;            // block_count + 1: block b holds chunks [first[b], first[b + 1]) of the new index
    std::vector<uint32_t> raw, tag;         // per block: the sum of its chunk sizes, its tag
    std::vector<uint64_t> stage;            // per block: where its chunks are staged, or NOWHERE (tag 0)
    std::vector<uint64_t> image, image_cap; // per block: where its image starts in the work buffer and the room it has
    std::vector<uint64_t> dest;             // per block: where its first chunk goes -- stage[b], or image[b] + header_bytes (tag 0)
    uint64_t staging_bytes = 0, work_bytes = 0, moved_bytes = 0;
};

// 0; EBADF: the blocks of `ni` do not list the chunks one after the other from 0 (no new index looks like that); EINVAL: a block whose
// chunk sizes sum to 4 GiB or more (a stored block records its raw size in 32 bits).  *why names the reason.
inline int layout(const restore_parse::StoreIndex& ni, Bound bound, Layout* out, const char** why)
{
    const uint32_t nb = ni.block_count;
    Layout& l = *out;
    l.first.assign((size_t)nb + 1, 0u), l.raw.assign(nb, 0u), l.tag.assign(nb, 0u);
    l.stage.assign(nb, NOWHERE), l.image.assign(nb, 0u), l.image_cap.assign(nb, 0u), l.dest.assign(nb, 0u);
    l.staging_bytes = l.work_bytes = l.moved_bytes = 0;
    uint64_t at = 0, staged = 0;
    for (uint32_t b = 0; b < nb; ++b)
    {
        const uint64_t off = ni.block_chunk_offsets[b], cnt = ni.block_chunk_counts[b];
        if (off != at || off + cnt > ni.chunk_count)
            return *why = "the new index's blocks do not list its chunks one after the other", EBADF;
        uint64_t raw = 0;
        for (uint64_t k = 0; k < cnt; ++k)
            raw += ni.chunk_sizes[off + k];
        if (raw > 0xFFFFFFFFull)
            return *why = "a new block's chunk sizes sum to 4 GiB or more", EINVAL;
        at += cnt;
        l.first[b + 1] = (uint32_t)at;
        l.raw[b] = (uint32_t)raw;
        l.tag[b] = ni.block_tags[b];
        l.moved_bytes += raw;
        if (l.tag[b])
        {
            l.stage[b] = staged;
            staged += raw;
        }
    }
    if (at != ni.chunk_count)
        return *why = "the new index holds chunks that no block lists", EBADF;
    l.staging_bytes = align8(staged);
    uint64_t end = l.staging_bytes;
    for (uint32_t b = 0; b < nb; ++b)
    {
        const uint32_t cnt = l.first[b + 1] - l.first[b];
        const uint64_t hdr = header_bytes(cnt, l.tag[b]);
        l.image[b] = end; // (8-byte aligned: staging_bytes is, and every image's room is rounded up)
        l.image_cap[b] = hdr + (l.tag[b] ? bound(l.tag[b], l.raw[b]) : (uint64_t)l.raw[b]);
        l.dest[b] = l.tag[b] ? l.stage[b] : l.image[b] + hdr;
        end += align8(l.image_cap[b]);
    }
    l.work_bytes = end;
    return 0;
}

// kept[b] = 1: block b of the store is named by the kept index (by hash; of store blocks that share a hash, all are kept)
inline void block_lists(const restore_parse::StoreIndex& store, const restore_parse::StoreIndex& kept_index, std::vector<uint8_t>* kept)
{
    std::unordered_map<uint64_t, uint32_t> held;
    for (uint32_t i = 0; i < kept_index.block_count; ++i)
        held.emplace(kept_index.block_hashes[i], i);
    kept->assign(store.block_count, 0);
    for (uint32_t b = 0; b < store.block_count; ++b)
        (*kept)[b] = held.count(store.block_hashes[b]) ? 1 : 0;
}

// The tag words of the serialized kept index `blob` (which parse_store_index accepted as `kept_index`) rewritten to what `store` records
// for the block of that hash (the first of blocks that share one).  Longtail_GetExistingStoreIndex takes a found block's tag from
// m_BlockTags[first chunk index] (src/longtail.c:7307), which lthip_get_existing_store_index mirrors: in a store of mixed tags that
// word is not the block's tag, and an index that carries it cannot be restored from.
inline void own_tags(const restore_parse::StoreIndex& store, const restore_parse::StoreIndex& kept_index, uint8_t* blob)
{
    std::unordered_map<uint64_t, uint32_t> block_of;
    for (uint32_t b = 0; b < store.block_count; ++b)
        block_of.emplace(store.block_hashes[b], b);
    uint8_t* tags = blob + (kept_index.block_tags.p - kept_index.block_hashes.p) + 16u;
    for (uint32_t i = 0; i < kept_index.block_count; ++i)
    {
        const auto it = block_of.find(kept_index.block_hashes[i]);
        if (it == block_of.end())
            continue;
        const uint32_t tag = store.block_tags[it->second];
        memcpy(tags + 4u * i, &tag, 4);
    }
}

} // namespace repack_plan
