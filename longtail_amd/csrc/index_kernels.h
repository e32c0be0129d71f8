// index_kernels.h -- the unique-index compaction of the first-seen pass (src/longtail.c:2951-2970): two small kernels shared by
// version_index.hip (the stand-alone VersionIndex call) and ingest.hip (the one-shot ingest session).  Included into both translation units.
#pragma once
#include "lthip_internal.h"

namespace
{
// is_first[i] = first_index[i] == i
__global__ void k_vi_mark(const uint32_t* __restrict__ first_index, uint64_t n, uint32_t* __restrict__ is_first)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        is_first[i] = first_index[i] == (uint32_t)i ? 1u : 0u;
}

// asset_chunk_indexes[i] = rank[first_index[i]]; first occurrences also fill the compact arrays
__global__ void k_vi_compact(const uint32_t* __restrict__ first_index, const uint32_t* __restrict__ rank, uint64_t n,
                             const uint64_t* __restrict__ hashes, const uint32_t* __restrict__ lens,
                             const uint32_t* __restrict__ asset_first_chunk /* [assets + 1] */, uint32_t asset_count,
                             const uint32_t* __restrict__ asset_tags /* may be null */, uint32_t* __restrict__ indexes,
                             uint64_t* __restrict__ uniq_hashes, uint32_t* __restrict__ uniq_sizes, uint32_t* __restrict__ uniq_tags)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t f = first_index[i];
    const uint32_t r = rank[f];
    indexes[i] = r;
    if (f == (uint32_t)i)
    {
        uniq_hashes[r] = hashes[i];
        uniq_sizes[r] = lens[i];
        uint32_t tag = 0;
        if (asset_tags)
        {
            uint32_t lo = 0, hi = asset_count; // asset a with asset_first_chunk[a] <= i < asset_first_chunk[a + 1]
            while (hi - lo > 1)
            {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (asset_first_chunk[mid] <= (uint32_t)i)
                    lo = mid;
                else
                    hi = mid;
            }
            tag = asset_tags[lo];
        }
        uniq_tags[r] = tag;
    }
}

} // namespace
