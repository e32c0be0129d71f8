// restore_windows.h -- byte windows of assets as occurrences of the restore session's write plan, on the host and without a line of HIP
// (include/longtail_hip.h, "byte windows of assets"), over restore_parse.h's reading of the VersionIndex.  The counterpart of the
// reference's ranged read (lib/blockstorestorage/longtail_blockstorestorage.c: BlockStoreStorageAPI_Read over ReadFromBlock).
//   expand        windows + a parsed VersionIndex -> per occurrence (chunk hash, FULL chunk length, skip, clip, destination).  A window
//                 [offset, offset + length) of asset a plans the chunks of a from the one that holds byte `offset` to the one that holds
//                 byte `offset + length - 1`, each clipped to the window: `skip` bytes into the chunk, `clip` bytes long, written at
//                 dst + (its first byte's position in the window).  The first and last chunk are found by bisection over the asset's
//                 chunk prefix sums, which are built once per asset that a PARTIAL window names: a small window into an asset of half
//                 a million chunks then costs one pass over that asset's chunk sizes, however many windows name it, and a window set
//                 of whole assets (lthip_restore_create's) builds no prefix sums at all and walks every chunk once, as before.
//                 A window of length 0 plans nothing; it still counts its asset as selected.
//   rank_windows  the jobs of one rank (lthip_make_jobs, lthip_partition_jobs) as windows into a dense output of that rank's own
//   asset_sizes   what an embedder needs to list a version's jobs when it holds the version as a blob
// The validation of lthip_restore_create_windows lives here; every refusal is EINVAL and names its reason.
// Included by restore.hip and by the stand-alone driver tests/san/restore_windows_driver.cpp.
#pragma once
#include "restore_parse.h"

#include <algorithm>
#include <vector>

namespace restore_windows
{

// lthip_restore_window (include/longtail_hip.h), restated so that this header stands alone
struct Window
{
    uint32_t asset, reserved;
    uint64_t offset, length, dst;
};
static_assert(sizeof(Window) == 32, "lthip_restore_window is 32 bytes");

constexpr uint64_t MAX_OCCURRENCES = 0x7FFFFFF0ull;

struct Occurrences
{
    std::vector<uint64_t> hash, dst;
    std::vector<uint32_t> len;        // the FULL length of the chunk: what the StoreIndex must hold it with
    std::vector<uint32_t> skip, clip; // empty when no window is partial: every occurrence is then (0, len)
    uint64_t assets_selected = 0;     // distinct assets named by a window of any length
};

// the chunks [first, last] of the asset that hold the window's first and last byte, and where chunk `first` starts in the asset;
// `pre`: the asset's chunk prefix sums (count + 1 entries), or null for a window that is the whole asset
inline void locate(const restore_parse::VersionIndex& v, const Window& w, const uint64_t* pre, uint64_t* first, uint64_t* last, uint64_t* begin)
{
    const uint64_t count = v.asset_chunk_counts[w.asset];
    if (!pre)
    {
        *first = 0, *last = count - 1u, *begin = 0;
        return;
    }
    // the last k with pre[k] <= x: chunk k is not empty and holds byte x (pre[0] = 0 <= x < pre[count] = the asset's size)
    const uint64_t* f = std::upper_bound(pre, pre + count + 1u, w.offset) - 1;
    const uint64_t* l = std::upper_bound(f, pre + count + 1u, w.offset + w.length - 1u) - 1;
    *first = (uint64_t)(f - pre), *last = (uint64_t)(l - pre), *begin = *f;
}

// 0, or EINVAL with *why set: windows == NULL with window_count > 0, asset >= asset_count, reserved != 0, offset + length beyond the
// asset's size, dst + length beyond out_bytes (both with overflow), more than MAX_OCCURRENCES occurrences in total (found before
// anything of that size is allocated).  May throw std::bad_alloc.
inline int expand(const restore_parse::VersionIndex& v, uint64_t window_count, const Window* windows, uint64_t out_bytes, Occurrences* out,
                  const char** why)
{
    const char* dummy;
    if (!why)
        why = &dummy;
    *why = "";
    if (window_count && !windows)
        return *why = "windows is NULL", EINVAL;
    constexpr uint64_t NO_PREFIX = ~0ull;
    std::vector<uint8_t> named(v.asset_count, 0);
    std::vector<uint64_t> pre_at; // per asset where its prefix sums start in `pre` (allocated when the first partial window is met)
    std::vector<uint64_t> pre;
    uint64_t total = 0;
    bool partial = false;
    // ---- pass 1: validate, count ----
    for (uint64_t i = 0; i < window_count; ++i)
    {
        const Window w = windows[i];
        if (w.asset >= v.asset_count)
            return *why = "a window names no asset of the version", EINVAL;
        if (w.reserved)
            return *why = "a window's reserved field is not 0", EINVAL;
        const uint64_t size = v.asset_sizes[w.asset];
        if (w.offset > size || w.length > size - w.offset)
            return *why = "a window leaves its asset", EINVAL;
        if (w.dst > out_bytes || w.length > out_bytes - w.dst)
            return *why = "a window leaves the output", EINVAL;
        if (!named[w.asset])
            named[w.asset] = 1, ++out->assets_selected;
        if (!w.length)
            continue;
        const uint64_t* p = nullptr;
        if (w.length != size) // (offset is then 0: the whole asset)
        {
            partial = true;
            if (pre_at.empty())
                pre_at.assign(v.asset_count, NO_PREFIX);
            if (pre_at[w.asset] == NO_PREFIX)
            {
                const uint64_t start = v.asset_chunk_index_starts[w.asset], count = v.asset_chunk_counts[w.asset];
                pre_at[w.asset] = pre.size();
                uint64_t at = 0; // (no reserve of the exact size here: it would copy `pre` once per asset)
                for (uint64_t k = 0; k < count; ++k)
                {
                    pre.push_back(at);
                    at += v.chunk_sizes[v.asset_chunk_indexes[start + k]];
                }
                pre.push_back(at);
            }
            p = pre.data() + pre_at[w.asset];
        }
        uint64_t first, last, begin;
        locate(v, w, p, &first, &last, &begin);
        total += last - first + 1u; // (2^64 is out of reach: every term is at most 2^32 and the sum is checked at every step)
        if (total > MAX_OCCURRENCES)
            return *why = "more than 0x7FFFFFF0 chunk writes in one session", EINVAL;
    }
    // ---- pass 2: the occurrences, window by window, chunk by chunk ----
    out->hash.reserve(total), out->dst.reserve(total), out->len.reserve(total);
    if (partial)
        out->skip.reserve(total), out->clip.reserve(total);
    for (uint64_t i = 0; i < window_count; ++i)
    {
        const Window w = windows[i];
        if (!w.length)
            continue;
        const uint64_t size = v.asset_sizes[w.asset], start = v.asset_chunk_index_starts[w.asset], end = w.offset + w.length;
        uint64_t first, last, at;
        locate(v, w, w.length != size ? pre.data() + pre_at[w.asset] : nullptr, &first, &last, &at);
        for (uint64_t k = first; k <= last; ++k)
        {
            const uint32_t c = v.asset_chunk_indexes[start + k];
            const uint32_t len = v.chunk_sizes[c];
            const uint64_t from = std::max(at, w.offset), to = std::min(at + len, end); // (from <= to: the chunk touches the window)
            out->hash.push_back(v.chunk_hashes[c]);
            out->len.push_back(len);
            out->dst.push_back(w.dst + (from - w.offset));
            if (partial)
            {
                out->skip.push_back((uint32_t)(from - at));
                out->clip.push_back((uint32_t)(to - from));
            }
            at += len;
        }
    }
    return 0;
}

// lthip_restore_asset_sizes: EINVAL a NULL blob, EBADF a malformed one; `sizes` may be NULL
inline int asset_sizes(const void* version_index, size_t size, uint64_t* sizes, uint32_t* asset_count, uint32_t* target_chunk_size)
{
    if (!version_index)
        return EINVAL;
    restore_parse::VersionIndex v;
    if (restore_parse::parse_version_index(version_index, size, &v))
        return EBADF;
    if (sizes)
        for (uint64_t a = 0; a < v.asset_count; ++a)
            sizes[a] = v.asset_sizes[a];
    if (asset_count)
        *asset_count = v.asset_count;
    if (target_chunk_size)
        *target_chunk_size = v.target_chunk_size;
    return 0;
}

// lthip_restore_rank_windows: the rank's non-empty jobs in job order; a job that continues the one before it (same asset, its offset the
// end of that one) joins its window; a window's dst is the end of the window before it rounded up to `align`.  EINVAL: `align` no power
// of two, window_count NULL, a NULL job array with job_count > 0, windows whose ends pass 2^64.  ENOMEM: `windows` given and `capacity`
// below the count (the count and *out_bytes are right either way).
inline int rank_windows(uint64_t job_count, const uint32_t* job_asset, const uint64_t* job_offset, const uint64_t* job_size,
                        const uint32_t* job_rank, uint32_t rank, uint64_t align, Window* windows, uint64_t capacity, uint64_t* window_count,
                        uint64_t* out_bytes)
{
    if (!window_count || align == 0 || (align & (align - 1u)) || (job_count && (!job_asset || !job_offset || !job_size || !job_rank)))
        return EINVAL;
    uint64_t n = 0, end = 0;
    for (int pass = 0; pass < 2; ++pass) // count, then (when they fit) write
    {
        if (pass && (!windows || n > capacity))
            break;
        n = 0, end = 0;
        Window cur = {0, 0, 0, 0, 0};
        bool open = false;
        for (uint64_t j = 0; j <= job_count; ++j)
        {
            if (j < job_count && (job_rank[j] != rank || !job_size[j]))
                continue;
            if (j < job_count && open && cur.asset == job_asset[j] && cur.offset + cur.length == job_offset[j])
            {
                if (end + job_size[j] < end)
                    return EINVAL;
                cur.length += job_size[j];
                end += job_size[j];
                continue;
            }
            if (open) // the window before this job is complete
            {
                if (pass)
                    windows[n] = cur;
                ++n;
            }
            if (j == job_count)
                break;
            const uint64_t start = (end + align - 1u) & ~(align - 1u);
            if (start < end || start + job_size[j] < start)
                return EINVAL;
            cur = Window{job_asset[j], 0u, job_offset[j], job_size[j], start};
            open = true;
            end = start + job_size[j];
        }
    }
    *window_count = n;
    if (out_bytes)
        *out_bytes = end;
    return windows && n > capacity ? ENOMEM : 0;
}

} // namespace restore_windows
