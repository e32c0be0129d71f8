// version_diff.h -- what changed between two serialized VersionIndexes, on the host and without a line of HIP: the lists of
// Longtail_CreateVersionDiff (src/longtail.c:7493-7756) over restore_parse.h's reading of the blobs.  Assets are matched by path hash:
// both versions' assets are put in ascending path-hash order and merged; a path hash only the source has is REMOVED, one only the target
// has is ADDED, one both have is content-modified when the content hashes differ and permissions-modified when the permissions do (an
// asset may be both).  The modified lists stay in the merge's order (ascending path hash, pair by pair); removed assets are then ordered
// by path length, longest first (a file before its directory), added ones shortest first (a directory before its files).  The
// reference leaves assets of equal path length to its qsort; here the sort is stable, so they stay in ascending path-hash order.
// Included by restore.hip (lthip_version_diff) and by the stand-alone driver tests/san/version_diff_driver.cpp.
#pragma once
#include "restore_parse.h"

#include <algorithm>
#include <vector>

namespace version_diff
{

struct Lists
{
    std::vector<uint32_t> source_removed, target_added, source_content, target_content, source_permissions, target_permissions;
};

// the assets of a version in ascending path-hash order; EBADF when two of them carry the same path hash
inline int by_path_hash(const restore_parse::VersionIndex& v, std::vector<uint32_t>* order)
{
    order->resize(v.asset_count);
    for (uint32_t a = 0; a < v.asset_count; ++a)
        (*order)[a] = a;
    std::sort(order->begin(), order->end(), [&v](uint32_t a, uint32_t b) { return v.path_hashes[a] < v.path_hashes[b]; });
    for (size_t i = 1; i < order->size(); ++i)
        if (v.path_hashes[(*order)[i]] == v.path_hashes[(*order)[i - 1]])
            return EBADF;
    return 0;
}

// 0; EBADF: a malformed blob, or two assets of one version with the same path hash; EINVAL: the hash identifiers differ
inline int diff(const void* source_vi, size_t source_size, const void* target_vi, size_t target_size, Lists* out)
{
    restore_parse::VersionIndex s, t;
    if (restore_parse::parse_version_index(source_vi, source_size, &s) || restore_parse::parse_version_index(target_vi, target_size, &t))
        return EBADF;
    if (s.hash_identifier != t.hash_identifier)
        return EINVAL;
    std::vector<uint32_t> so, to;
    if (by_path_hash(s, &so) || by_path_hash(t, &to))
        return EBADF;
    size_t i = 0, j = 0;
    while (i < so.size() || j < to.size())
    {
        const bool has_s = i < so.size(), has_t = j < to.size();
        const uint64_t hs = has_s ? s.path_hashes[so[i]] : 0, ht = has_t ? t.path_hashes[to[j]] : 0;
        if (has_s && has_t && hs == ht)
        {
            const uint32_t a = so[i++], b = to[j++];
            if (s.content_hashes[a] != t.content_hashes[b])
                out->source_content.push_back(a), out->target_content.push_back(b);
            if (s.permissions[a] != t.permissions[b])
                out->source_permissions.push_back(a), out->target_permissions.push_back(b);
        }
        else if (has_s && (!has_t || hs < ht))
            out->source_removed.push_back(so[i++]);
        else
            out->target_added.push_back(to[j++]);
    }
    std::vector<uint32_t> slen(s.asset_count), tlen(t.asset_count);
    for (const uint32_t a : out->source_removed)
        slen[a] = s.path_length(a);
    for (const uint32_t b : out->target_added)
        tlen[b] = t.path_length(b);
    std::stable_sort(out->source_removed.begin(), out->source_removed.end(), [&slen](uint32_t a, uint32_t b) { return slen[a] > slen[b]; });
    std::stable_sort(out->target_added.begin(), out->target_added.end(), [&tlen](uint32_t a, uint32_t b) { return tlen[a] < tlen[b]; });
    return 0;
}

} // namespace version_diff
