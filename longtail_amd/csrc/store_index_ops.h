// store_index_ops.h -- the two operations that keep a store's index in step with its blocks, on the host and without a line of HIP:
//   prune  Longtail_PruneStoreIndex (src/longtail.c:9287-9421): the blocks of an index whose hash is in a keep list, in the index's order
//   merge  Longtail_MergeStoreIndex (:9151-9285): the blocks of `local`, then the blocks of `remote` that `local` does not hold
// each followed by Longtail_WriteStoreIndexToBuffer: the output is the serialized StoreIndex (layout :8913-8931), byte for byte the
// reference's.  What is mirrored, quirks included:
//   prune  a block hash that stands twice in the index is kept twice (the reference looks the KEEP list up, not the index); repeats and
//          unknown hashes in the keep list change nothing; the hash identifier is the source's even when no block is kept.
//   merge  local blocks first, in their order; a block hash is taken once and its FIRST occurrence gives the tag and the chunk list, so a
//          block both sides hold is local's.  The hash identifier is local's when local has blocks, else remote's when remote has
//          blocks, else 0 (Longtail_CreateStoreIndexFromBlocks(0, 0)); EINVAL when BOTH have blocks and their identifiers differ --
//          the rule looks at block counts, not chunk counts, as the reference does.
// Also version_chunk_hashes: the chunk hashes of a serialized VersionIndex, in its order -- the live set of a version a caller keeps.
// The inputs are untrusted bytes of any alignment and go through restore_parse.h, which refuses (EBADF) what is short, of another
// version or inconsistent; the output may lie at any alignment too, every word is written with memcpy.  Counts are summed in 64 bits:
// a result whose block or chunk count does not fit the 32 bits of the header is EINVAL, not truncated.  Input and output must not
// overlap.  Included by lthip_ctx.hip (lthip_store_index_prune / _merge, lthip_version_chunk_hashes) and by the stand-alone driver
// tests/san/store_index_ops_driver.cpp.
#pragma once
#include "restore_parse.h"

#include <unordered_set>
#include <vector>

namespace store_index_ops
{

using restore_parse::StoreIndex;

// the bytes of a serialized StoreIndex of these counts (Longtail_GetStoreIndexDataSize): below 2^37 for 32-bit counts
inline uint64_t store_index_bytes(uint64_t nb, uint64_t m) { return 16u + 20u * nb + 12u * m; }

// one block of the result: block `block` of index `from`
struct Pick
{
    const StoreIndex* from;
    uint32_t block;
};

// The picked blocks in turn as one serialized StoreIndex.  *out_size = its bytes (whenever they fit a header); ENOMEM, nothing
// written: `out` is null or `capacity` is below that.
inline int write_picks(uint32_t hash_identifier, const std::vector<Pick>& picks, void* out, size_t capacity, size_t* out_size)
{
    const uint64_t nb = picks.size();
    uint64_t m = 0;
    for (const Pick& p : picks)
        m += p.from->block_chunk_counts[p.block];
    if (nb > 0xFFFFFFFFull || m > 0xFFFFFFFFull)
        return EINVAL;
    const uint64_t bytes = store_index_bytes(nb, m);
    if (bytes > (uint64_t)SIZE_MAX)
        return EINVAL;
    *out_size = (size_t)bytes;
    if (!out || (uint64_t)capacity < bytes)
        return ENOMEM;
    uint8_t* w = (uint8_t*)out;
    const uint32_t head[4] = {restore_parse::STORE_INDEX_VERSION, hash_identifier, (uint32_t)nb, (uint32_t)m};
    memcpy(w, head, 16);
    uint8_t* block_hashes = w + 16;
    uint8_t* chunk_hashes = block_hashes + nb * 8u;
    uint8_t* block_offsets = chunk_hashes + m * 8u;
    uint8_t* block_counts = block_offsets + nb * 4u;
    uint8_t* block_tags = block_counts + nb * 4u;
    uint8_t* chunk_sizes = block_tags + nb * 4u;
    uint32_t at = 0;
    for (uint64_t b = 0; b < nb; ++b)
    {
        const StoreIndex& s = *picks[b].from;
        const uint32_t block = picks[b].block, first = s.block_chunk_offsets[block], count = s.block_chunk_counts[block], tag = s.block_tags[block];
        memcpy(block_hashes + b * 8u, s.block_hashes.p + (uint64_t)block * 8u, 8);
        memcpy(block_offsets + b * 4u, &at, 4);
        memcpy(block_counts + b * 4u, &count, 4);
        memcpy(block_tags + b * 4u, &tag, 4);
        if (count) // (parse_store_index has placed [first, first + count) inside the chunk arrays)
        {
            memcpy(chunk_hashes + (uint64_t)at * 8u, s.chunk_hashes.p + (uint64_t)first * 8u, (size_t)count * 8u);
            memcpy(chunk_sizes + (uint64_t)at * 4u, s.chunk_sizes.p + (uint64_t)first * 4u, (size_t)count * 4u);
        }
        at += count;
    }
    return 0;
}

// 0; EINVAL: a null index or size pointer, a keep count without a list; EBADF: restore_parse refuses the blob; ENOMEM with *out_size
// set: `out` is null or too small.  keep_block_hashes is the caller's array (aligned), keep_count entries.
inline int prune(const void* store_index, size_t size, uint32_t keep_count, const uint64_t* keep_block_hashes, void* out, size_t capacity, size_t* out_size)
{
    if (!store_index || !out_size || (keep_count && !keep_block_hashes))
        return EINVAL;
    StoreIndex s;
    if (restore_parse::parse_store_index(store_index, size, &s))
        return EBADF;
    const std::unordered_set<uint64_t> keep(keep_block_hashes, keep_block_hashes + keep_count);
    std::vector<Pick> picks;
    for (uint32_t b = 0; b < s.block_count; ++b)
        if (keep.count(s.block_hashes[b]))
            picks.push_back(Pick{&s, b});
    return write_picks(s.hash_identifier, picks, out, capacity, out_size);
}

// 0; EINVAL: a null pointer, or both indexes have blocks and name different hash types; EBADF: restore_parse refuses a blob; ENOMEM
// with *out_size set: `out` is null or too small.
inline int merge(const void* local, size_t local_size, const void* remote, size_t remote_size, void* out, size_t capacity, size_t* out_size)
{
    if (!local || !remote || !out_size)
        return EINVAL;
    StoreIndex l, r;
    if (restore_parse::parse_store_index(local, local_size, &l) || restore_parse::parse_store_index(remote, remote_size, &r))
        return EBADF;
    uint32_t hash_identifier = 0;
    if (l.block_count == 0)
        hash_identifier = r.block_count ? r.hash_identifier : 0u;
    else
    {
        hash_identifier = l.hash_identifier;
        if (r.block_count && r.hash_identifier != hash_identifier)
            return EINVAL;
    }
    std::unordered_set<uint64_t> seen;
    seen.reserve((size_t)l.block_count + r.block_count);
    std::vector<Pick> picks;
    for (const StoreIndex* s : {&l, &r})
        for (uint32_t b = 0; b < s->block_count; ++b)
            if (seen.insert(s->block_hashes[b]).second)
                picks.push_back(Pick{s, b});
    return write_picks(hash_identifier, picks, out, capacity, out_size);
}

// The chunk hashes of a serialized VersionIndex, in its order (every hash once: a VersionIndex lists its distinct chunks).  *count = how
// many there are; `out` (the caller's array, `capacity` entries) may be null to ask for the count alone.  EINVAL: a null blob or count
// pointer; EBADF: restore_parse refuses the blob; ENOMEM with *count set: `out` is null or too small, nothing written.
inline int version_chunk_hashes(const void* version_index, size_t size, uint64_t* out, uint64_t capacity, uint64_t* count)
{
    if (!version_index || !count)
        return EINVAL;
    restore_parse::VersionIndex v;
    if (restore_parse::parse_version_index(version_index, size, &v))
        return EBADF;
    *count = v.chunk_count;
    if (!out || capacity < v.chunk_count)
        return v.chunk_count ? ENOMEM : 0;
    if (v.chunk_count)
        memcpy(out, v.chunk_hashes.p, (size_t)v.chunk_count * 8u);
    return 0;
}

} // namespace store_index_ops
