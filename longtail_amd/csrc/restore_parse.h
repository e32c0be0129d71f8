// restore_parse.h -- reading the two serialized indexes a restore starts from, on the host and without a line of HIP: the VersionIndex
// (layout src/longtail.c:2551-2584) and the StoreIndex (:8913-8931).  A blob is untrusted bytes of any alignment: every word is read
// with memcpy, every array is placed by 64-bit arithmetic on 32-bit counts (which cannot overflow) and checked against the blob's size
// before it is touched, and every index read from the blob is checked before it is used.  Anything short, of another version or
// inconsistent is EBADF.  Included by restore.hip, by version_diff.h and by the stand-alone driver tests/san/restore_parse_driver.cpp.
#pragma once
#include <errno.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace restore_parse
{

constexpr uint32_t VERSION_INDEX_VERSION = 2u;      // LONGTAIL_VERSION_INDEX_VERSION_0_0_2 (src/longtail.c:16-22)
constexpr uint32_t STORE_INDEX_VERSION = 1u << 24;  // LONGTAIL_STORE_INDEX_VERSION_1_0_0
constexpr uint64_t SKIP = ~0ull;                    // LTHIP_RESTORE_SKIP

// The hash types longtail has (lib/blake2, lib/blake3, lib/meowhash): a restore verifies chunks with the type the indexes name, so an
// identifier that names none of them is as malformed as a wrong version.
inline bool known_hash_identifier(uint32_t id) { return id == 0x626c6b32u /*'blk2'*/ || id == 0x626c6b33u /*'blk3'*/ || id == 0x6d656f77u /*'meow'*/; }

// an array of the blob: element i by memcpy (the blob has any alignment)
struct U32s
{
    const uint8_t* p = nullptr;
    uint32_t operator[](uint64_t i) const
    {
        uint32_t v;
        memcpy(&v, p + i * 4u, 4);
        return v;
    }
};
struct U64s
{
    const uint8_t* p = nullptr;
    uint64_t operator[](uint64_t i) const
    {
        uint64_t v;
        memcpy(&v, p + i * 8u, 8);
        return v;
    }
};
struct U16s
{
    const uint8_t* p = nullptr;
    uint16_t operator[](uint64_t i) const
    {
        uint16_t v;
        memcpy(&v, p + i * 2u, 2);
        return v;
    }
};

struct VersionIndex
{
    uint32_t hash_identifier = 0, target_chunk_size = 0, asset_count = 0, chunk_count = 0, asset_chunk_index_count = 0;
    U64s path_hashes, content_hashes;                       // [asset_count]
    U64s asset_sizes;                                       // [asset_count]
    U32s asset_chunk_counts, asset_chunk_index_starts;      // [asset_count]
    U32s asset_chunk_indexes;                               // [asset_chunk_index_count]
    U64s chunk_hashes;                                      // [chunk_count]
    U32s chunk_sizes;                                       // [chunk_count]
    U32s name_offsets;                                      // [asset_count] into name_data
    U16s permissions;                                       // [asset_count]
    const uint8_t* name_data = nullptr;                     // the rest of the blob
    uint64_t name_data_size = 0;
    // strlen of asset a's path (parse_version_index has found its terminator inside the name data)
    uint32_t path_length(uint64_t a) const { return (uint32_t)strlen((const char*)name_data + name_offsets[a]); }
};

struct StoreIndex
{
    uint32_t hash_identifier = 0, block_count = 0, chunk_count = 0;
    U64s block_hashes;                                      // [block_count]
    U64s chunk_hashes;                                      // [chunk_count]
    U32s block_chunk_offsets, block_chunk_counts, block_tags; // [block_count]
    U32s chunk_sizes;                                       // [chunk_count]
};

// 0, or EBADF: shorter than its arrays, another version, a hash identifier that names no hash type, a target chunk size whose largest
// chunk (twice the target, src/longtail.c:1985-1987) does not fit the 32 bits of a chunk size, fewer chunk indexes than chunks
// (Longtail_GetVersionIndexDataSize refuses it), an asset whose path does not start and end inside the name data, an asset whose
// chunk-index run leaves the index array, a chunk index that names no chunk, an asset whose chunk sizes do not sum to its size.  Path
// and content hashes and permissions are placed and handed out (the blob must hold them; version_diff.h reads them), tags are placed
// but not read.
inline int parse_version_index(const void* blob, size_t size, VersionIndex* out)
{
    if (!blob || size < 24)
        return EBADF;
    const uint8_t* p = (const uint8_t*)blob;
    U32s head;
    head.p = p;
    if (head[0] != VERSION_INDEX_VERSION)
        return EBADF;
    VersionIndex v;
    v.hash_identifier = head[1];
    v.target_chunk_size = head[2];
    v.asset_count = head[3];
    v.chunk_count = head[4];
    v.asset_chunk_index_count = head[5];
    if (!known_hash_identifier(v.hash_identifier) || v.target_chunk_size > 0x7FFFFFFFu)
        return EBADF;
    const uint64_t na = v.asset_count, nu = v.chunk_count, ni = v.asset_chunk_index_count;
    if (ni < nu)
        return EBADF;
    // 24 + na * (8 + 8 + 8 + 4 + 4) + ni * 4 + nu * (8 + 4 + 4) + na * (4 + 2): below 2^40 for any 32-bit counts
    const uint64_t need = 24u + na * 32u + ni * 4u + nu * 16u + na * 6u;
    if ((uint64_t)size < need)
        return EBADF;
    uint64_t o = 24u;
    v.path_hashes.p = p + o;
    o += na * 8u;
    v.content_hashes.p = p + o;
    o += na * 8u;
    v.asset_sizes.p = p + o;
    o += na * 8u;
    v.asset_chunk_counts.p = p + o;
    o += na * 4u;
    v.asset_chunk_index_starts.p = p + o;
    o += na * 4u;
    v.asset_chunk_indexes.p = p + o;
    o += ni * 4u;
    v.chunk_hashes.p = p + o;
    o += nu * 8u;
    v.chunk_sizes.p = p + o;
    o += nu * 8u; // (m_ChunkSizes, m_ChunkTags)
    v.name_offsets.p = p + o;
    o += na * 4u;
    v.permissions.p = p + o;
    o += na * 2u;
    v.name_data = p + o;
    v.name_data_size = (uint64_t)size - o;
    for (uint64_t a = 0; a < na; ++a)
    {
        // the asset's path: a string that starts and ends inside the name data (which is what is left of the blob: a blob cut short
        // anywhere loses at least the last path's terminator)
        const uint64_t name = v.name_offsets[a];
        if (name >= v.name_data_size || !memchr(v.name_data + name, 0, (size_t)(v.name_data_size - name)))
            return EBADF;
        const uint64_t start = v.asset_chunk_index_starts[a], count = v.asset_chunk_counts[a];
        if (start + count > ni)
            return EBADF;
        uint64_t sum = 0; // (at most 2^32 terms below 2^32)
        for (uint64_t k = 0; k < count; ++k)
        {
            const uint32_t c = v.asset_chunk_indexes[start + k];
            if (c >= nu)
                return EBADF;
            sum += v.chunk_sizes[c];
        }
        if (sum != v.asset_sizes[a])
            return EBADF;
    }
    *out = v;
    return 0;
}

// 0, or EBADF: shorter than its arrays, another version than 1.0.0, a hash identifier that names no hash type (an index without chunks
// carries 0, src/longtail.c:6931-6943), a block whose chunk run leaves the chunk arrays or whose chunk sizes
// sum to 4 GiB or more (a stored block records its raw size in 32 bits)
inline int parse_store_index(const void* blob, size_t size, StoreIndex* out)
{
    if (!blob || size < 16)
        return EBADF;
    const uint8_t* p = (const uint8_t*)blob;
    U32s head;
    head.p = p;
    if (head[0] != STORE_INDEX_VERSION)
        return EBADF;
    StoreIndex s;
    s.hash_identifier = head[1];
    s.block_count = head[2];
    s.chunk_count = head[3];
    const uint64_t nb = s.block_count, m = s.chunk_count;
    if (!known_hash_identifier(s.hash_identifier) && !(s.hash_identifier == 0u && m == 0u))
        return EBADF;
    if ((uint64_t)size < 16u + nb * 20u + m * 12u)
        return EBADF;
    uint64_t o = 16;
    s.block_hashes.p = p + o;
    o += nb * 8u;
    s.chunk_hashes.p = p + o;
    o += m * 8u;
    s.block_chunk_offsets.p = p + o;
    o += nb * 4u;
    s.block_chunk_counts.p = p + o;
    o += nb * 4u;
    s.block_tags.p = p + o;
    o += nb * 4u;
    s.chunk_sizes.p = p + o;
    for (uint64_t b = 0; b < nb; ++b)
    {
        const uint64_t first = s.block_chunk_offsets[b], count = s.block_chunk_counts[b];
        if (first + count > m)
            return EBADF;
        uint64_t raw = 0;
        for (uint64_t k = 0; k < count; ++k)
            raw += s.chunk_sizes[first + k];
        if (raw > 0xFFFFFFFFull)
            return EBADF;
    }
    *out = s;
    return 0;
}

// The dense layout of a version's assets at `align`-byte boundaries (a power of two): asset_offsets[a] (may be null) = where asset a
// starts = the end of the asset before it rounded up to `align`, *total_bytes = the end of the last asset.  Directories and empty
// files take no room: they get the offset an asset of any size would get there.
inline int layout(const VersionIndex& v, uint64_t align, uint64_t* asset_offsets, uint64_t* total_bytes)
{
    if (align == 0 || (align & (align - 1u)))
        return EINVAL;
    uint64_t at = 0;
    for (uint64_t a = 0; a < v.asset_count; ++a)
    {
        const uint64_t size = v.asset_sizes[a];
        const uint64_t start = (at + align - 1u) & ~(align - 1u);
        if (start < at || start + size < start)
            return EBADF; // (sizes that sum past 2^64: no such version)
        if (asset_offsets)
            asset_offsets[a] = start;
        at = start + size;
    }
    if (total_bytes)
        *total_bytes = at;
    return 0;
}

} // namespace restore_parse
