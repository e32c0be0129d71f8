// index_kernels.h -- the tail of Longtail_CreateVersionIndex as steps that version_index.hip (the stand-alone VersionIndex call) and
// ingest.hip (the one-shot ingest session) share: the builder's workspace, step 1 -- the unique-index compaction of the first-seen pass
// (src/longtail.c:2951-2970), two small kernels and their launches, here because both translation units carry the kernels -- and the
// declarations of the refusals and of steps 2 and 3 (version_index.hip).  Included into both translation units.
#pragma once
#include "lthip_internal.h"
#include "ingest_buffers.h"

// the builder's device tables, grown and kept: a session holds one, lthip_build_version_index a local one
struct ViWorkspace
{
    DBuf d_isfirst, d_rank, d_idx, d_uh, d_us, d_ut, d_starts, d_tags, d_paths, d_aoff, d_alen, d_ph, d_ch;
};
// the tree as the builder reads it: host arrays of `na` assets; counts = the chunks of every asset, starts = their exclusive sum (na + 1)
struct ViTree
{
    uint32_t na;
    const uint64_t* asset_sizes;
    const uint32_t* path_offsets;
    const uint16_t* permissions;
    const char* path_data;
    uint32_t path_data_size;
    const uint32_t *counts, *starts;
    uint32_t hash_identifier, target_chunk_size;
};
int lthip_vi_reserve(lthip_ctx* ctx, ViWorkspace& w, uint64_t n, uint32_t na, uint32_t path_data_size);
// what the builder does not take -- an asset with more than 2^29 chunks, a path offset outside the path data: EINVAL under the name
// `who`, before any work is queued
int lthip_vi_refusals(lthip_ctx* ctx, const ViTree& t, const char* who);
// step 2: content hash of every asset over the `n` chunk hashes, path hashes -- tables uploaded and two hash launches on ctx's stream
int lthip_vi_hashes(lthip_ctx* ctx, ViWorkspace& w, const ViTree& t, const uint64_t* d_chunk_hashes, uint32_t n);
// step 3: header and all sections of the serialized VersionIndex into `out` (lthip_version_index_size bytes), device sections copied
// on ctx's stream and not waited for.  one_tag != null: the tag column is that constant instead of the device list
int lthip_vi_sections(lthip_ctx* ctx, const ViWorkspace& w, const ViTree& t, uint32_t n, uint64_t unique, const uint32_t* one_tag, void* out);

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

// step 1: the asset starts (and tags, may be null) uploaded, then mark, scan and compact on ctx's stream: from a device first-seen index
// of the n chunks -- however it was obtained -- the unique index of every asset chunk (d_idx) and the unique lists (d_uh / d_us / d_ut)
int vi_unique_lists(lthip_ctx* ctx, ViWorkspace& w, const uint32_t* d_first, uint32_t n, const uint64_t* d_hashes, const uint32_t* d_lens,
                    const uint32_t* starts, const uint32_t* tags, uint32_t na)
{
    hipStream_t s = ctx->stream;
    int err;
    if ((err = lthip_stage_upload(ctx, w.d_starts.p, starts, ((size_t)na + 1) * 4, s)) || (tags && (err = lthip_stage_upload(ctx, w.d_tags.p, tags, (size_t)na * 4, s))))
        return err;
    if (!n)
        return 0;
    const uint32_t blocks = (uint32_t)div_up_u64(n, 256);
    LaunchTimer tm(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_vi_mark, dim3(blocks), dim3(256), 0, s, d_first, (uint64_t)n, (uint32_t*)w.d_isfirst.p);
    if ((err = lthip_exclusive_scan_u32(ctx, (const uint32_t*)w.d_isfirst.p, (uint32_t*)w.d_rank.p, n, nullptr, LTHIP_K_OTHER)))
        return err;
    hipLaunchKernelGGL(k_vi_compact, dim3(blocks), dim3(256), 0, s, d_first, (const uint32_t*)w.d_rank.p, (uint64_t)n, d_hashes, d_lens,
                       (const uint32_t*)w.d_starts.p, na, tags ? (const uint32_t*)w.d_tags.p : (const uint32_t*)nullptr, (uint32_t*)w.d_idx.p,
                       (uint64_t*)w.d_uh.p, (uint32_t*)w.d_us.p, (uint32_t*)w.d_ut.p);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

} // namespace
