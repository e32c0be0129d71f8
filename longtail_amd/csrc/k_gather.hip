// k_gather.hip -- block assembly on the device: WriteContentBlockJob builds a stored block by
// reading every chunk of the block into one contiguous buffer (src/longtail.c:4640-4721).  With the assets already
// resident in HBM that is a gather of byte ranges: one workgroup per chunk, copied by lthip_wg_copy (k_copy.h).
// Only needed when a block is not already one contiguous range of the asset buffer (dedup holes,
// assets whose sizes are not multiples of 16).
#include "k_copy.h"
#include "lthip_internal.h"
#include "store_layout.h"

#include <algorithm>
#include <vector>

namespace
{

constexpr int GT = 256;

__global__ __launch_bounds__(GT) void k_gather_ranges(const uint8_t* __restrict__ src, const uint64_t* __restrict__ src_offsets,
                                                      const uint32_t* __restrict__ lens, const uint64_t* __restrict__ dst_offsets,
                                                      uint64_t count, uint8_t* __restrict__ dst)
{
    const uint64_t i = blockIdx.x;
    if (i >= count)
        return;
    const uint8_t* s = src + src_offsets[i];
    uint8_t* d = dst + dst_offsets[i];
    lthip_wg_copy<GT>(d, s, lens[i], threadIdx.x);
}

// Pinned host memory <-> HBM by the CUs.  The box's SDMA engines move ONE direction at a time (tools/pcie_duplex_probe.py,
// profiles/r05_pcie_duplex.json: hipMemcpyAsync h2d + d2h on two streams take the SUM of their times, 57 GB/s in total), a kernel
// that loads / stores over the link does not share them: kernel copies in both directions at once reach 46 GB/s EACH.  A host-fed
// ingest loop therefore fetches its slices and returns its block images with this kernel (and lthip_gather_ranges, whose
// destination may be pinned host memory too), on streams of their own beside the compute stream.
__global__ __launch_bounds__(GT) void k_link_copy(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t nvec, uint32_t tail)
{
    const uint64_t stride = (uint64_t)gridDim.x * GT;
    uint64_t v = (uint64_t)blockIdx.x * GT + threadIdx.x;
    for (; v + 3u * stride < nvec; v += 4u * stride) // four 16-byte requests of every lane in flight (1 KiB per wave and request)
    {
        const uint4 a = src[v], b = src[v + stride], c = src[v + 2u * stride], d = src[v + 3u * stride];
        dst[v] = a;
        dst[v + stride] = b;
        dst[v + 2u * stride] = c;
        dst[v + 3u * stride] = d;
    }
    for (; v < nvec; v += stride)
        dst[v] = src[v];
    if (blockIdx.x == 0 && threadIdx.x < tail)
        reinterpret_cast<uint8_t*>(dst + nvec)[threadIdx.x] = reinterpret_cast<const uint8_t*>(src + nvec)[threadIdx.x];
}

// positions of a rank's chunks in job order (the multi-GPU exchange): chunk k of the rank lies in its own job m with
// part_first[m] <= k < part_first[m + 1] (lthip_chunk_hash's part table: one part per own job, ascending) and is the tree's chunk
// job_gfirst[m] + (k - part_first[m])
__global__ void k_job_ordinals(const uint32_t* __restrict__ part_first, uint32_t nparts, const uint32_t* __restrict__ job_gfirst,
                               uint32_t nlocal, uint32_t* __restrict__ out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nlocal)
        return;
    uint32_t lo = 0, hi = nparts; // (empty parts: the last one that starts at or before k)
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (part_first[mid] <= k)
            lo = mid;
        else
            hi = mid;
    }
    out[k] = job_gfirst[lo] + (k - part_first[lo]);
}

// ---- raw block images: the payload of a block with tag 0 is its chunks' bytes as they are (CompressBlock, compressblockstore.c:85-90) ----
// A pure copy of N bytes to where the images lie: the payload starts 20 + 12 n bytes into an 8-aligned image, the chunks follow each other
// at any byte position.  The unit of work is a bounded PIECE of a RUN -- a maximal stretch of a block's chunks that is contiguous in the
// source (a block that is one byte range of the data is one run) -- and a unit belongs to a wave, so a run of 48 bytes costs a wave
// a few instructions and not a workgroup, and an 8 MiB run spreads over 256 waves.
//
//   k_raw_runs   a wave per block walks its chunk list 64 chunks at a time: destination of every chunk (prefix sum of the lengths), run
//                starts (a chunk that does not continue the one before), and per run {source, destination, length} in the slot of its
//                first chunk; every other slot of the block gets 0 pieces
//   scan         pieces of the slots -> first piece of every slot (lthip_exclusive_scan_u32)
//   k_raw_copy   a fixed grid of waves strides over the pieces; a piece finds its slot by bisection of the scan (scalar loads)
// (the size of a piece, LTHIP_RAW_PIECE_VEC, and the pieces of a run, lthip_raw_pieces: lthip_internal.h -- the restore session's carry
// forms runs of its own)
__global__ __launch_bounds__(64) void k_raw_runs(const uint64_t* __restrict__ blk_payload, const uint32_t* __restrict__ blk_first,
                                                 const uint32_t* __restrict__ blk_count, uint32_t nblocks, uint32_t chunk_base,
                                                 const uint32_t* __restrict__ lens, const uint64_t* __restrict__ src_offsets,
                                                 uint64_t* __restrict__ run_src, uint64_t* __restrict__ run_dst, uint64_t* __restrict__ run_len,
                                                 uint32_t* __restrict__ pieces)
{
    const uint32_t b = blockIdx.x;
    if (b >= nblocks)
        return;
    const uint32_t lane = threadIdx.x;
    const uint32_t c0 = blk_first[b], n = blk_count[b];
    uint64_t pos = blk_payload[b]; // destination of the group's first chunk
    uint64_t prev_end = 0;          // source end of the chunk before the group
    bool open = false;              // a run that began in an earlier group and has not ended
    uint32_t open_slot = 0;
    uint64_t open_dst = 0;
    for (uint32_t g = 0; g < n; g += 64)
    {
        const uint32_t i = g + lane;
        const bool valid = i < n;
        const uint32_t len = valid ? lens[c0 + i] : 0u;
        const uint64_t so = valid ? src_offsets[c0 + i] : 0ull;
        uint64_t incl = len; // inclusive prefix sum over the wave
        for (int o = 1; o < 64; o <<= 1)
        {
            const uint64_t up = __shfl_up(incl, o, 64);
            if ((int)lane >= o)
                incl += up;
        }
        const uint64_t dst = pos + incl - len, end = so + len;
        uint64_t before = __shfl_up(end, 1, 64);
        if (lane == 0)
            before = prev_end;
        const bool start = valid && (i == 0 || so != before);
        const uint64_t mask = __ballot(start);
        // every start finds the next one in the group: that is where its run ends; the last start of the group stays open
        const uint64_t above = lane < 63 ? mask & ~((2ull << lane) - 1ull) : 0ull;
        const uint32_t next = start && above ? (uint32_t)__ffsll((unsigned long long)above) - 1u : lane;
        const uint64_t next_dst = __shfl(dst, (int)next, 64);
        if (mask)
        {
            const uint32_t f = (uint32_t)__ffsll((unsigned long long)mask) - 1u, l = 63u - (uint32_t)__clzll((long long)mask);
            const uint64_t first_dst = __shfl(dst, (int)f, 64), last_dst = __shfl(dst, (int)l, 64);
            if (open && lane == 0) // the run carried in ends at the group's first start
            {
                run_len[open_slot] = first_dst - open_dst;
                pieces[open_slot] = lthip_raw_pieces(open_dst, first_dst - open_dst);
            }
            open = true;
            open_slot = c0 + g + l - chunk_base;
            open_dst = last_dst;
        }
        if (valid)
        {
            const uint32_t slot = c0 + i - chunk_base;
            uint32_t np = 0;
            if (start)
            {
                run_src[slot] = so;
                run_dst[slot] = dst;
                if (above)
                {
                    run_len[slot] = next_dst - dst;
                    np = lthip_raw_pieces(dst, next_dst - dst);
                }
            }
            if (!start || above) // (the open run's slot is written when it ends)
                pieces[slot] = np;
        }
        const uint32_t last_valid = n - g < 64u ? n - g - 1u : 63u;
        pos += __shfl(incl, 63, 64);
        prev_end = __shfl(end, (int)last_valid, 64);
    }
    if (open && lane == 0)
    {
        run_len[open_slot] = pos - open_dst;
        pieces[open_slot] = lthip_raw_pieces(open_dst, pos - open_dst);
    }
}

__global__ __launch_bounds__(GT) void k_raw_copy(const uint32_t* __restrict__ first_piece /* [slots + 1] */, uint32_t slots,
                                                 const uint64_t* __restrict__ run_src, const uint64_t* __restrict__ run_dst,
                                                 const uint64_t* __restrict__ run_len, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t waves = gridDim.x * (GT / 64u);
    const uint32_t total = first_piece[slots];
    for (uint32_t u = blockIdx.x * (GT / 64u) + wave; u < total; u += waves)
    {
        uint32_t lo = 0, hi = slots; // first_piece[lo] <= u < first_piece[hi]: the slot that owns piece u (empty slots: the last such)
        while (hi - lo > 1)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (first_piece[mid] <= u)
                lo = mid;
            else
                hi = mid;
        }
        const uint32_t p = u - first_piece[lo], np = first_piece[lo + 1] - first_piece[lo];
        const uint8_t* s = src + run_src[lo];
        uint8_t* d = dst + run_dst[lo];
        uint64_t n = run_len[lo];
        uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);
        if (head > n)
            head = (uint32_t)n;
        if (p == 0 && lane < head)
            d[lane] = s[lane];
        d += head;
        s += head;
        n -= head;
        const uint64_t nvec = n >> 4;
        const uint32_t tail = (uint32_t)(n & 15u);
        if (p == np - 1 && lane < tail)
            d[(nvec << 4) + lane] = s[(nvec << 4) + lane];
        // the piece's share of the run's vectors: equal parts
        const uint64_t v0 = nvec * p / np, v1 = nvec * (p + 1u) / np;
        const uint32_t mis = (uint32_t)((uintptr_t)s & 3u), sh = mis * 8u;
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s - mis);
        uint64_t v = v0 + lane;
        for (; v + 192u < v1; v += 256u) // four 16-byte requests of every lane in flight (1 KiB per wave and request)
        {
            const RawVec a = raw_load(s4 + v * 4u, mis), b = raw_load(s4 + (v + 64u) * 4u, mis), c = raw_load(s4 + (v + 128u) * 4u, mis),
                         e = raw_load(s4 + (v + 192u) * 4u, mis);
            *reinterpret_cast<uint4*>(d + v * 16u) = raw_align(a, sh);
            *reinterpret_cast<uint4*>(d + (v + 64u) * 16u) = raw_align(b, sh);
            *reinterpret_cast<uint4*>(d + (v + 128u) * 16u) = raw_align(c, sh);
            *reinterpret_cast<uint4*>(d + (v + 192u) * 16u) = raw_align(e, sh);
        }
        for (; v < v1; v += 64u)
            *reinterpret_cast<uint4*>(d + v * 16u) = raw_align(raw_load(s4 + v * 4u, mis), sh);
    }
}

// element ranges -> byte ranges of k_gather_ranges
__global__ void k_scale_ranges(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst, const uint32_t* __restrict__ cnt,
                               uint64_t count, uint32_t elem_bytes, uint64_t* __restrict__ src_b, uint64_t* __restrict__ dst_b,
                               uint32_t* __restrict__ len_b)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count)
        return;
    src_b[i] = src[i] * elem_bytes;
    dst_b[i] = dst[i] * elem_bytes;
    len_b[i] = cnt[i] * elem_bytes;
}

} // namespace

extern "C" int lthip_exchange_reorder(lthip_ctx* ctx, const void* d_gathered, void* d_out, uint32_t elem_bytes, uint64_t range_count,
                                      const uint64_t* range_src, const uint64_t* range_dst, const uint32_t* range_cnt)
{
    if (!ctx || !elem_bytes || (range_count && (!d_gathered || !d_out || !range_src || !range_dst || !range_cnt)))
        return EINVAL;
    if (range_count == 0)
        return 0;
    if (range_count > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "lthip_exchange_reorder", "too many ranges");
    // k_scale_ranges holds a range's length in bytes in 32 bits (k_gather_ranges' table format): a range of count * elem_bytes above
    // that would be copied in part, silently -- refused instead (lthip_exchange_ranges cuts ranges at max_piece ELEMENTS; a caller
    // that passes a large max_piece with 8-byte elements lands here)
    for (uint64_t i = 0; i < range_count; ++i)
        if ((uint64_t)range_cnt[i] * elem_bytes > 0xFFFFFFFFull)
            return lthip_fail(ctx, EINVAL, "lthip_exchange_reorder", "a range of more than 4 GiB - 1 bytes: cut the ranges smaller (max_piece)");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    // tables: {src, dst} u64 + cnt u32 in elements, then the same in bytes
    const size_t n = (size_t)range_count, n8 = (n + 1) & ~(size_t)1;
    void* tab = nullptr;
    int err = lthip_scratch(ctx, S_XCHG, n8 * 40 + 64, &tab);
    if (err)
        return err;
    uint64_t* d_src = (uint64_t*)tab;
    uint64_t* d_dst = d_src + n8;
    uint64_t* d_src_b = d_dst + n8;
    uint64_t* d_dst_b = d_src_b + n8;
    uint32_t* d_cnt = (uint32_t*)(d_dst_b + n8);
    uint32_t* d_len_b = d_cnt + n8;
    hipStream_t s = ctx->stream;
    if ((err = lthip_stage_upload(ctx, d_src, range_src, n * 8, s)) || (err = lthip_stage_upload(ctx, d_dst, range_dst, n * 8, s)) ||
        (err = lthip_stage_upload(ctx, d_cnt, range_cnt, n * 4, s)))
        return err;
    LaunchTimer t(ctx, LTHIP_K_GATHER);
    hipLaunchKernelGGL(k_scale_ranges, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, d_src, d_dst, d_cnt, (uint64_t)n, elem_bytes,
                       d_src_b, d_dst_b, d_len_b);
    hipLaunchKernelGGL(k_gather_ranges, dim3((uint32_t)n), dim3(GT), 0, s, (const uint8_t*)d_gathered, d_src_b, d_len_b, d_dst_b,
                       (uint64_t)n, (uint8_t*)d_out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

int lthip_raw_copy_runs(lthip_ctx* ctx, const uint32_t* d_first_piece, uint32_t slots, const uint64_t* d_run_src, const uint64_t* d_run_dst,
                        const uint64_t* d_run_len, const void* d_src, void* d_dst, uint64_t pieces_bound)
{
    if (slots == 0)
        return 0;
    // a fixed grid strides over the pieces (their number is on the device): eight workgroups per CU at most, fewer when the pieces are few
    uint64_t grid = 2048;
    if (pieces_bound)
        grid = std::min<uint64_t>(grid, div_up_u64(pieces_bound, GT / 64u));
    LaunchTimer t(ctx, LTHIP_K_GATHER);
    hipLaunchKernelGGL(k_raw_copy, dim3((uint32_t)grid), dim3(GT), 0, ctx->stream, d_first_piece, slots, d_run_src, d_run_dst, d_run_len,
                       (const uint8_t*)d_src, (uint8_t*)d_dst);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

int lthip_raw_copy_blocks(lthip_ctx* ctx, uint32_t count, const uint32_t* h_first, const uint32_t* h_count, const uint64_t* h_payload,
                          uint32_t chunk_base, uint32_t chunk_span, const uint32_t* d_lens, const uint64_t* d_src_offsets, const void* d_src,
                          void* d_arena, uint64_t bytes_bound)
{
    if (count == 0 || chunk_span == 0)
        return 0;
    hipStream_t s = ctx->stream;
    // block tables: [count u64 payload][count u32 first][count u32 chunks], one upload
    const size_t k = count, span = chunk_span, span2 = (span + 2) & ~(size_t)1;
    std::vector<uint64_t> tab(k * 2);
    memcpy(tab.data(), h_payload, k * 8);
    memcpy((uint32_t*)(tab.data() + k), h_first, k * 4);
    memcpy((uint32_t*)(tab.data() + k) + k, h_count, k * 4);
    void *blocks = nullptr, *runs = nullptr;
    int err;
    if ((err = lthip_scratch(ctx, S_RAW_BLOCKS, k * 16, &blocks)) || (err = lthip_scratch(ctx, S_RAW_RUNS, span2 * 32, &runs)) ||
        (err = lthip_stage_upload(ctx, blocks, tab.data(), k * 16, s)))
        return err;
    const uint64_t* d_payload = (const uint64_t*)blocks;
    const uint32_t* d_first = (const uint32_t*)(d_payload + k);
    const uint32_t* d_count = d_first + k;
    uint64_t* run_src = (uint64_t*)runs; // one slot per chunk of the span
    uint64_t* run_dst = run_src + span2;
    uint64_t* run_len = run_dst + span2;
    uint32_t* pieces = (uint32_t*)(run_len + span2);
    uint32_t* first_piece = pieces + span2; // [span + 1]
    LTHIP_CHECK(ctx, hipMemsetAsync(pieces, 0, span * 4, s)); // (chunks of the span that are in none of these blocks)
    {
        LaunchTimer t(ctx, LTHIP_K_GATHER);
        hipLaunchKernelGGL(k_raw_runs, dim3(count), dim3(64), 0, s, d_payload, d_first, d_count, count, chunk_base, d_lens, d_src_offsets,
                           run_src, run_dst, run_len, pieces);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if ((err = lthip_exclusive_scan_u32(ctx, pieces, first_piece, span, nullptr, LTHIP_K_GATHER)))
        return err;
    return lthip_raw_copy_runs(ctx, first_piece, chunk_span, run_src, run_dst, run_len, d_src, d_arena,
                               bytes_bound ? bytes_bound / (LTHIP_RAW_PIECE_VEC * 16u) + span + k : 0);
}

extern "C" int lthip_write_raw_block_images(lthip_ctx* ctx, uint32_t block_count, const uint64_t* block_first_chunk, const uint64_t* d_chunk_hashes,
                                            const uint32_t* d_chunk_lens, const uint64_t* d_chunk_src_offsets, const void* d_src,
                                            uint32_t hash_identifier, void* d_arena, const uint64_t* image_offsets)
{
    if (!ctx || (block_count && (!block_first_chunk || !d_chunk_hashes || !d_chunk_lens || !d_chunk_src_offsets || !d_src || !d_arena || !image_offsets)))
        return EINVAL;
    if (block_count == 0)
        return 0;
    const size_t nb = block_count;
    std::vector<uint32_t> first(nb + 1), cnt(nb);
    std::vector<uint64_t> payload(nb);
    for (size_t b = 0; b <= nb; ++b)
    {
        if (block_first_chunk[b] > 0x7FFFFFF0ull || (b && block_first_chunk[b] < block_first_chunk[b - 1]))
            return lthip_fail(ctx, EINVAL, "raw block images", "block_first_chunk must be non-decreasing and below 2^31");
        first[b] = (uint32_t)block_first_chunk[b];
    }
    for (size_t b = 0; b < nb; ++b)
    {
        if (image_offsets[b] & 7u)
            return lthip_fail(ctx, EINVAL, "raw block images", "image offsets must be 8-byte aligned");
        cnt[b] = first[b + 1] - first[b];
        if ((uint64_t)cnt[b] * 8u > 0xFFFFFFFFull)
            return lthip_fail(ctx, EINVAL, "raw block images", "a block of more than 2^29 chunks");
        payload[b] = image_offsets[b] + lthip_block_index_size(cnt[b]);
    }
    BlockHashRanges r;
    r.fill(first.data(), nb, 0);
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    // ---- the payloads first: the copy is the long part, the BlockIndex kernel runs behind it ----
    int err;
    if ((err = lthip_raw_copy_blocks(ctx, block_count, first.data(), cnt.data(), payload.data(), first[0], first[nb] - first[0], d_chunk_lens,
                                     d_chunk_src_offsets, d_src, d_arena, 0)))
        return err;
    // ---- block hashes = hash of each block's chunk-hash array (:3753-3757), then the BlockIndex in front of every payload ----
    const size_t nb2 = (nb + 2) & ~(size_t)1;
    void* tabs = nullptr;
    if ((err = lthip_scratch(ctx, S_RAW_TABLES, nb2 * 32, &tabs)))
        return err;
    uint64_t* d_off = (uint64_t*)tabs;
    uint64_t* d_img = d_off + nb2;
    uint64_t* d_bh = d_img + nb2;
    uint32_t* d_len = (uint32_t*)(d_bh + nb2);
    uint32_t* d_firstc = d_len + nb2; // [nb + 1]
    if ((err = lthip_stage_upload(ctx, d_off, r.off.data(), nb * 8, s)) || (err = lthip_stage_upload(ctx, d_img, image_offsets, nb * 8, s)) ||
        (err = lthip_stage_upload(ctx, d_len, r.len.data(), nb * 4, s)) || (err = lthip_stage_upload(ctx, d_firstc, first.data(), (nb + 1) * 4, s)))
        return err;
    if ((err = lthip_hash_ranges_by_id(ctx, hash_identifier, d_chunk_hashes, nb, d_off, d_len, r.max_len, r.leaves, d_bh)))
        return err;
    return lthip_launch_block_headers(ctx, LTHIP_K_GATHER, d_firstc, block_count, d_chunk_hashes, d_chunk_lens, d_bh, hash_identifier, 0u, nullptr, nullptr,
                                      nullptr, d_img, d_arena, 1u);
}

extern "C" int lthip_job_ordinals(lthip_ctx* ctx, uint64_t my_job_count, const uint32_t* local_first, const uint32_t* global_first,
                                  uint64_t local_chunks, uint32_t* d_out)
{
    if (!ctx || (local_chunks && (!my_job_count || !local_first || !global_first || !d_out)))
        return EINVAL;
    if (local_chunks == 0)
        return 0;
    if (local_chunks > 0x7FFFFFF0ull || my_job_count > 0x7FFFFFF0ull)
        return lthip_fail(ctx, EINVAL, "lthip_job_ordinals", "counts out of range");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t m = (size_t)my_job_count;
    void* tab = nullptr;
    int err = lthip_scratch(ctx, S_XCHG2, m * 8 + 64, &tab);
    if (err)
        return err;
    uint32_t* d_lf = (uint32_t*)tab;
    uint32_t* d_gf = d_lf + m;
    hipStream_t s = ctx->stream;
    if ((err = lthip_stage_upload(ctx, d_lf, local_first, m * 4, s)) || (err = lthip_stage_upload(ctx, d_gf, global_first, m * 4, s)))
        return err;
    LaunchTimer t(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_job_ordinals, dim3((uint32_t)((local_chunks + 255) / 256)), dim3(256), 0, s, d_lf, (uint32_t)m, d_gf,
                       (uint32_t)local_chunks, d_out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int lthip_gather_ranges(lthip_ctx* ctx, const void* d_src, uint64_t range_count, const uint64_t* d_src_offsets,
                                   const uint32_t* d_lens, void* d_dst, const uint64_t* d_dst_offsets)
{
    if (!ctx || (range_count && (!d_src || !d_src_offsets || !d_lens || !d_dst || !d_dst_offsets)))
        return EINVAL;
    if (range_count == 0)
        return 0;
    if (range_count > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "gather", "too many ranges");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LaunchTimer t(ctx, LTHIP_K_GATHER);
    hipLaunchKernelGGL(k_gather_ranges, dim3((uint32_t)range_count), dim3(GT), 0, ctx->stream, (const uint8_t*)d_src,
                       d_src_offsets, d_lens, d_dst_offsets, range_count, (uint8_t*)d_dst);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int lthip_link_copy(lthip_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx || (bytes && (!dst || !src)))
        return EINVAL;
    if (bytes == 0)
        return 0;
    if (((uintptr_t)dst | (uintptr_t)src) & 15u)
        return lthip_fail(ctx, EINVAL, "lthip_link_copy", "source and destination must be 16-byte aligned");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t nvec = (uint64_t)bytes >> 4;
    uint64_t grid = div_up_u64(nvec ? nvec : 1, (uint64_t)GT * 4u);
    if (grid > 1024)
        grid = 1024; // (enough requests in flight for the link; the waves mostly wait, the compute stream's kernels run beside them)
    LaunchTimer t(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_link_copy, dim3((uint32_t)grid), dim3(GT), 0, ctx->stream, (const uint4*)src, (uint4*)dst, nvec, (uint32_t)(bytes & 15u));
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}
