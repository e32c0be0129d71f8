// restore_layout.h -- where the assets of a target version go in the buffer a base version lies restored in, on the host and without a
// line of HIP: the layout of an update IN PLACE (include/longtail_hip.h, "updating a resident version in place"), over restore_parse.h's
// reading of the blobs and version_diff.h's order by path hash.  The rule is deterministic:
//   * assets are matched by path hash.  A target asset of size > 0 is KEPT when the base has a resident asset (offset != SKIP) with the
//     same path hash, size and content hash: it gets that asset's offset
//   * the GAPS are [0, base_bytes) minus the kept windows, ascending, each with a cursor at its start
//   * every other target asset of size > 0, in asset order, goes into the first gap where round_up(cursor, align) + size <= the gap's
//     end, and the cursor moves to the asset's end
//   * an asset that fits no gap is appended at round_up(end, align), where `end` starts at base_bytes
//   * assets of size 0 (directories, empty files) get offset 0
//   * total = the highest end of any target window (it may lie below base_bytes)
// A new asset may land on the old bytes of a modified one: lthip_restore_carry_in_place reads everything it moves before it writes.
// First fit walks the gaps from the first that still has room, so the cost is assets x open gaps at worst.
// Included by restore.hip (lthip_restore_layout_in_place) and by the stand-alone driver tests/san/restore_layout_driver.cpp.
#pragma once
#include "version_diff.h"

namespace restore_layout
{

struct Gap
{
    uint64_t cursor, end;
};

// 0; EINVAL: `align` no power of two, a null blob or null base_offsets, hash identifiers that differ, a resident base asset outside
// [0, base_bytes), two kept windows that overlap; EBADF: a malformed blob, two assets of one version with the same path hash (or sizes
// that sum past 2^64: no such version).  Every output may be null.
inline int in_place(const void* base_vi, size_t base_size, const uint64_t* base_offsets, uint64_t base_bytes, const void* target_vi,
                    size_t target_size, uint64_t align, uint64_t* target_offsets, uint32_t* asset_count, uint64_t* total_bytes,
                    uint32_t* kept_assets)
{
    if (!base_vi || !target_vi || !base_offsets || align == 0 || (align & (align - 1u)))
        return EINVAL;
    restore_parse::VersionIndex b, t;
    if (restore_parse::parse_version_index(base_vi, base_size, &b) || restore_parse::parse_version_index(target_vi, target_size, &t))
        return EBADF;
    if (b.hash_identifier != t.hash_identifier)
        return EINVAL;
    std::vector<uint32_t> bo, to;
    if (version_diff::by_path_hash(b, &bo) || version_diff::by_path_hash(t, &to))
        return EBADF;
    for (uint64_t a = 0; a < b.asset_count; ++a)
    {
        const uint64_t off = base_offsets[a], size = b.asset_sizes[a];
        if (off != restore_parse::SKIP && size && (off > base_bytes || size > base_bytes - off))
            return EINVAL;
    }
    // ---- kept: the merge of the two orders; where[k] = the offset target asset k keeps, or SKIP ----
    std::vector<uint64_t> where(t.asset_count, restore_parse::SKIP);
    std::vector<Gap> kept; // (the kept windows first, then turned into the gaps between them)
    for (size_t i = 0, j = 0; i < bo.size() && j < to.size();)
    {
        const uint64_t hb = b.path_hashes[bo[i]], ht = t.path_hashes[to[j]];
        if (hb < ht)
            ++i;
        else if (ht < hb)
            ++j;
        else
        {
            const uint32_t x = bo[i++], y = to[j++];
            const uint64_t size = t.asset_sizes[y];
            if (size && base_offsets[x] != restore_parse::SKIP && b.asset_sizes[x] == size && b.content_hashes[x] == t.content_hashes[y])
            {
                where[y] = base_offsets[x];
                kept.push_back(Gap{base_offsets[x], base_offsets[x] + size});
            }
        }
    }
    std::sort(kept.begin(), kept.end(), [](const Gap& p, const Gap& q) { return p.cursor < q.cursor; });
    for (size_t k = 1; k < kept.size(); ++k)
        if (kept[k].cursor < kept[k - 1].end)
            return EINVAL;
    std::vector<Gap> gaps;
    uint64_t at = 0;
    for (const Gap& w : kept)
    {
        if (w.cursor > at)
            gaps.push_back(Gap{at, w.cursor});
        at = w.end;
    }
    if (base_bytes > at)
        gaps.push_back(Gap{at, base_bytes});
    // ---- everything else: first fit in asset order, or appended ----
    uint64_t end = base_bytes, total = 0;
    size_t open = 0; // the gaps before it are full
    for (uint64_t a = 0; a < t.asset_count; ++a)
    {
        const uint64_t size = t.asset_sizes[a];
        uint64_t off = 0;
        if (size && where[a] != restore_parse::SKIP)
            off = where[a];
        else if (size)
        {
            bool placed = false;
            while (open < gaps.size() && gaps[open].cursor == gaps[open].end)
                ++open;
            for (size_t g = open; g < gaps.size() && !placed; ++g)
            {
                const uint64_t start = (gaps[g].cursor + align - 1u) & ~(align - 1u);
                if (start < gaps[g].cursor || start > gaps[g].end || size > gaps[g].end - start)
                    continue;
                off = start;
                gaps[g].cursor = start + size;
                placed = true;
            }
            if (!placed)
            {
                const uint64_t start = (end + align - 1u) & ~(align - 1u);
                if (start < end || start + size < start)
                    return EBADF;
                off = start;
                end = start + size;
            }
        }
        if (size && off + size > total)
            total = off + size;
        if (target_offsets)
            target_offsets[a] = off;
    }
    if (asset_count)
        *asset_count = t.asset_count;
    if (total_bytes)
        *total_bytes = total;
    if (kept_assets)
        *kept_assets = (uint32_t)kept.size();
    return 0;
}

} // namespace restore_layout
