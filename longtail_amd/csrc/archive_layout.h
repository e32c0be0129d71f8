// archive_layout.h -- the index of a one-file archive, on the host and without a line of HIP: the file golongtail's pack / unpack move
// around is [ArchiveIndex][block][block]... (Longtail_CreateArchiveIndex / Longtail_ReadArchiveIndex, src/longtail.c:9921-10090;
// lib/archiveblockstore/longtail_archiveblockstore.c).  The index, exactly as the reference writes it:
//   u32 version (LONGTAIL_VERSION(0,0,1))   u32 index_data_size (of the WHOLE index, these eight bytes included)
//   the serialized StoreIndex, 16 + 20 nb + 12 m bytes
//   u64 block_start_offsets[nb], relative to the end of the index      u32 block_sizes[nb]
//   the serialized VersionIndex      padding to a multiple of 8
// index_data_size = (8 + S + 12 nb + V + 7) & 0xfffffff8 in 32 bits (:9945): an index that does not fit 32 bits is refused, not
// truncated.  The u64 table starts at byte 24 + 20 nb + 12 m, which is only 4-byte aligned when nb + m is odd: every word is read and
// written with memcpy.  The reference leaves the pad bytes uninitialised; ours are zero.  A serialized VersionIndex does not store the
// length of its name data, so a reader takes "the rest of the index" as the VersionIndex (:10075-10082), pad included:
// restore_parse::parse_version_index takes the name data as what is left of the blob and accepts the up to 7 trailing bytes.
// Blocks lie in the body in ANY order (the reference writes them as its workers complete, archiveblockstore.c:70-77) and at any byte
// position; that they overlap is not an error, every image is checked against the StoreIndex when it is delivered.
// Included by archive.hip, restore.hip, restore_call.h and the stand-alone driver tests/san/archive_driver.cpp.
#pragma once
#include "restore_parse.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace archive_layout
{

constexpr uint32_t ARCHIVE_VERSION = 1u;        // LONGTAIL_ARCHIVE_VERSION_0_0_1 (src/longtail.c:20)
constexpr uint64_t BODY_UNKNOWN = ~0ull;        // open(): the body's size is not known
constexpr uint64_t MIN_INDEX_BYTES = 8u + 16u + 24u; // the head, a StoreIndex without blocks, a VersionIndex without assets

inline uint32_t get32(const uint8_t* p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
inline uint64_t get64(const uint8_t* p)
{
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}
inline void put32(uint8_t* p, uint32_t v) { memcpy(p, &v, 4); }
inline void put64(uint8_t* p, uint64_t v) { memcpy(p, &v, 8); }

// the bytes of a serialized StoreIndex of these counts (Longtail_GetStoreIndexDataSize): below 2^37
inline uint64_t store_index_bytes(uint64_t nb, uint64_t m) { return 16u + 20u * nb + 12u * m; }
// the header a stored block of n chunks starts with: the BlockIndex, and [raw size][compressed size] when it carries a tag
inline uint64_t block_header_bytes(uint64_t n, uint32_t tag) { return 20u + 12u * n + (tag ? 8u : 0u); }

// The size of the index of these two blobs.  EBADF: a blob restore_parse calls malformed; EINVAL: the index would not fit 32 bits.
inline int index_size(const void* si, size_t si_size, const void* vi, size_t vi_size, uint64_t* out_bytes, restore_parse::StoreIndex* out_si = nullptr)
{
    restore_parse::StoreIndex s;
    restore_parse::VersionIndex v;
    if (restore_parse::parse_store_index(si, si_size, &s) || restore_parse::parse_version_index(vi, vi_size, &v))
        return EBADF;
    const uint64_t nb = s.block_count;
    if ((uint64_t)vi_size > 0xFFFFFFFFull)
        return EINVAL;
    const uint64_t bytes = 8u + store_index_bytes(nb, s.chunk_count) + 12u * nb + (uint64_t)vi_size; // (below 2^38)
    if (bytes + 7u > 0xFFFFFFFFull)
        return EINVAL;
    if (out_bytes)
        *out_bytes = (bytes + 7u) & ~(uint64_t)7u;
    if (out_si)
        *out_si = s;
    return 0;
}

// Writes the index of the two blobs with these tables (nb entries each, host) into out[0, capacity).  ENOMEM: capacity below
// index_size(); nothing is written then.
inline int write_index(const void* si, size_t si_size, const void* vi, size_t vi_size, const uint64_t* block_offsets, const uint32_t* block_sizes,
                       void* out, size_t capacity)
{
    uint64_t bytes = 0;
    restore_parse::StoreIndex s;
    const int err = index_size(si, si_size, vi, vi_size, &bytes, &s);
    if (err)
        return err;
    const uint64_t nb = s.block_count, sb = store_index_bytes(nb, s.chunk_count);
    if (!out || (nb && (!block_offsets || !block_sizes)))
        return EINVAL;
    if ((uint64_t)capacity < bytes)
        return ENOMEM;
    uint8_t* p = (uint8_t*)out;
    put32(p, ARCHIVE_VERSION);
    put32(p + 4, (uint32_t)bytes);
    p += 8;
    memcpy(p, si, (size_t)sb);
    p += sb;
    for (uint64_t b = 0; b < nb; ++b)
        put64(p + 8u * b, block_offsets[b]);
    p += 8u * nb;
    for (uint64_t b = 0; b < nb; ++b)
        put32(p + 4u * b, block_sizes[b]);
    p += 4u * nb;
    memcpy(p, vi, vi_size);
    p += vi_size;
    memset(p, 0, (size_t)((uint8_t*)out + bytes - p));
    return 0;
}

// The first eight bytes of an archive -> the bytes of its index.  EBADF: another version, or a size no index has.
inline int peek(const void* first_8_bytes, uint64_t* index_bytes)
{
    if (!first_8_bytes || !index_bytes)
        return EINVAL;
    const uint8_t* p = (const uint8_t*)first_8_bytes;
    if (get32(p) != ARCHIVE_VERSION || get32(p + 4) < MIN_INDEX_BYTES)
        return EBADF;
    *index_bytes = get32(p + 4);
    return 0;
}

// An opened archive: a copy of the index, where its parts lie in it, and the two tables as host arrays.
struct Archive
{
    std::vector<uint8_t> index;
    uint64_t si_at = 0, si_bytes = 0, vi_at = 0, vi_bytes = 0; // vi_bytes: the rest of the index, pad included
    uint64_t body_bytes = 0;                                   // as given, or (BODY_UNKNOWN) the end of the last block
    uint32_t hash_identifier = 0;
    std::vector<uint64_t> offsets, bhash;
    std::vector<uint32_t> sizes;
};

// 0, or EBADF: index_bytes is not the size the index stores (a short or over-long index), another version, counts that leave the
// index, a StoreIndex or VersionIndex that restore_parse calls malformed, a block smaller than its own header, a block whose
// offset + size leaves body_bytes (or, with BODY_UNKNOWN, 2^64).
inline int open(const void* index, size_t index_bytes, uint64_t body_bytes, Archive* out)
{
    if (!index || !out)
        return EINVAL;
    uint64_t stored = 0;
    if (index_bytes < 8 || peek(index, &stored) || stored != (uint64_t)index_bytes)
        return EBADF;
    const uint8_t* p = (const uint8_t*)index;
    restore_parse::StoreIndex s;
    if (restore_parse::parse_store_index(p + 8, index_bytes - 8, &s))
        return EBADF;
    const uint64_t nb = s.block_count, sb = store_index_bytes(nb, s.chunk_count);
    const uint64_t tables_at = 8u + sb, vi_at = tables_at + 12u * nb;
    if (vi_at > (uint64_t)index_bytes)
        return EBADF;
    restore_parse::VersionIndex v;
    if (restore_parse::parse_version_index(p + vi_at, (size_t)(index_bytes - vi_at), &v))
        return EBADF;
    Archive a;
    a.offsets.resize(nb), a.sizes.resize(nb), a.bhash.resize(nb);
    uint64_t end = 0;
    for (uint64_t b = 0; b < nb; ++b)
    {
        const uint64_t off = get64(p + tables_at + 8u * b), size = get32(p + tables_at + 8u * nb + 4u * b);
        if (size < block_header_bytes(s.block_chunk_counts[b], s.block_tags[b]))
            return EBADF;
        if (off + size < off || (body_bytes != BODY_UNKNOWN && (off > body_bytes || size > body_bytes - off)))
            return EBADF;
        end = std::max(end, off + size);
        a.offsets[b] = off, a.sizes[b] = (uint32_t)size, a.bhash[b] = s.block_hashes[b];
    }
    a.index.assign(p, p + index_bytes);
    a.si_at = 8, a.si_bytes = sb, a.vi_at = vi_at, a.vi_bytes = (uint64_t)index_bytes - vi_at;
    a.body_bytes = body_bytes == BODY_UNKNOWN ? end : body_bytes;
    a.hash_identifier = s.hash_identifier;
    *out = std::move(a);
    return 0;
}

// Body ranges {first byte, bytes}: sorted by their first byte and merged where the gap between one's end and the next's start is at most
// max_gap (ranges that touch or overlap always merge).  What a reader of a few files out of a large archive reads.
inline void merge_ranges(std::vector<std::pair<uint64_t, uint64_t>>* ranges, uint64_t max_gap)
{
    std::sort(ranges->begin(), ranges->end());
    size_t k = 0;
    for (size_t i = 0; i < ranges->size(); ++i)
    {
        const std::pair<uint64_t, uint64_t> r = (*ranges)[i];
        if (k)
        {
            std::pair<uint64_t, uint64_t>& last = (*ranges)[k - 1];
            const uint64_t last_end = last.first + last.second;
            if (r.first <= last_end || r.first - last_end <= max_gap)
            {
                last.second = std::max(last_end, r.first + r.second) - last.first;
                continue;
            }
        }
        (*ranges)[k++] = r;
    }
    ranges->resize(k);
}

} // namespace archive_layout

// the handle of the C interface (include/longtail_hip.h, "one-file archives")
struct lthip_archive
{
    archive_layout::Archive a;
};
