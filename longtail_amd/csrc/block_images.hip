// block_images.hip -- the block writer of the ingest sessions: a batch of packed blocks (BlockBatch, ingest_buffers.h) becomes
// stored-block images in the caller's arena (Longtail_WriteContent, src/longtail.c:4760).  First the payloads: a raw block's chunks are
// copied from where they lie to behind its BlockIndex, every other block is compressed straight to image + header size, one codec call
// per (codec, zstd quality) key and place the sources lie in.  Then, once the block hashes are queued, BlockIndex + [raw][compressed]
// around them (:4111-4150; compressblockstore.c:103-139).  Nothing here waits, and nothing is allocated once the session's tables
// (BlockImageBufs) have grown to their size.
#include "lthip_internal.h"
#include "ingest_buffers.h"

namespace
{
// BlockIndex (+ the size words of a compressed payload) of every block's image.  raw_mode != 0: a block whose tag is 0 is a RAW image
// (CompressBlock passes it through, compressblockstore.c:85-90: BlockIndex, then the chunks' bytes) -- it gets no [raw][compressed]
// words, raw_sizes is not read for it, and comp_sizes[b] (when not null) RECEIVES the sum of its chunk lengths: what the sessions
// count and report as its stored payload size.  With raw_mode == 0 comp_sizes is only read.
__global__ __launch_bounds__(64) void k_stored_block_headers(const uint32_t* __restrict__ block_first_chunk /* [nblocks + 1] */,
                                                             uint32_t nblocks, const uint64_t* __restrict__ chunk_hashes,
                                                             const uint32_t* __restrict__ chunk_lens,
                                                             const uint64_t* __restrict__ block_hashes, uint32_t hash_identifier,
                                                             uint32_t tag, const uint32_t* __restrict__ block_tags /* null: `tag` */,
                                                             const uint32_t* __restrict__ raw_sizes, uint32_t* comp_sizes,
                                                             const uint64_t* __restrict__ image_offsets, uint8_t* __restrict__ arena,
                                                             uint32_t raw_mode)
{
    const uint32_t b = blockIdx.x;
    if (b >= nblocks)
        return;
    const uint32_t c0 = block_first_chunk[b], n = block_first_chunk[b + 1] - c0;
    uint8_t* w = arena + image_offsets[b]; // 8-byte aligned by contract
    const int lane = threadIdx.x;
    const uint32_t btag = block_tags ? block_tags[b] : tag;
    if (lane == 0)
    {
        *reinterpret_cast<uint64_t*>(w) = block_hashes[b];
        uint32_t* h = reinterpret_cast<uint32_t*>(w + 8);
        h[0] = hash_identifier;
        h[1] = n;
        h[2] = btag;
    }
    uint8_t* hashes = w + 20; // only 4-byte aligned
    for (uint32_t i = lane; i < n; i += 64)
    {
        const uint64_t v = chunk_hashes[c0 + i];
        uint32_t* p = reinterpret_cast<uint32_t*>(hashes + (size_t)i * 8);
        p[0] = (uint32_t)v;
        p[1] = (uint32_t)(v >> 32);
    }
    uint32_t* sizes = reinterpret_cast<uint32_t*>(hashes + (size_t)n * 8);
    uint32_t sum = 0;
    for (uint32_t i = lane; i < n; i += 64)
    {
        const uint32_t l = chunk_lens[c0 + i];
        sizes[i] = l;
        sum += l;
    }
    if (raw_mode && btag == 0u)
    {
        if (comp_sizes) // (wave-uniform: b and the tag are the block's)
        {
            for (int o = 32; o > 0; o >>= 1)
                sum += __shfl_down(sum, o, 64);
            if (lane == 0)
                comp_sizes[b] = sum;
        }
        return;
    }
    if (lane == 0)
    {
        sizes[n] = raw_sizes[b];
        sizes[n + 1] = comp_sizes[b];
    }
}
} // namespace

int lthip_launch_block_headers(lthip_ctx* ctx, int kid, const uint32_t* d_block_first_chunk, uint32_t nblocks, const uint64_t* d_chunk_hashes,
                               const uint32_t* d_chunk_lens, const uint64_t* d_block_hashes, uint32_t hash_identifier, uint32_t tag,
                               const uint32_t* d_block_tags, const uint32_t* d_raw_sizes, uint32_t* d_comp_sizes, const uint64_t* d_image_offsets,
                               void* d_arena, uint32_t raw_mode)
{
    LaunchTimer tm(ctx, kid);
    hipLaunchKernelGGL(k_stored_block_headers, dim3(nblocks), dim3(64), 0, ctx->stream, d_block_first_chunk, nblocks, d_chunk_hashes, d_chunk_lens,
                       d_block_hashes, hash_identifier, tag, d_block_tags, d_raw_sizes, d_comp_sizes, d_image_offsets, (uint8_t*)d_arena, raw_mode);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

int lthip_gather_upload(lthip_ctx* ctx, BlockImageBufs& w, const void* d_src, const Ranges& r, void* d_dst)
{
    const size_t k = r.src.size();
    if (!k)
        return 0;
    int err;
    // (the tables of the call before this one were read by a kernel queued before these uploads: the stream orders them)
    if ((err = reserve_dev(ctx, w.d_gsrc, k * 8)) || (err = reserve_dev(ctx, w.d_glen, k * 4)) || (err = reserve_dev(ctx, w.d_gdst, k * 8)) ||
        (err = lthip_stage_upload(ctx, w.d_gsrc.p, r.src.data(), k * 8, ctx->stream)) ||
        (err = lthip_stage_upload(ctx, w.d_glen.p, r.len.data(), k * 4, ctx->stream)) ||
        (err = lthip_stage_upload(ctx, w.d_gdst.p, r.dst.data(), k * 8, ctx->stream)))
        return err;
    return lthip_gather_ranges(ctx, d_src, k, (const uint64_t*)w.d_gsrc.p, (const uint32_t*)w.d_glen.p, d_dst, (const uint64_t*)w.d_gdst.p);
}

int lthip_block_payloads(lthip_ctx* ctx, BlockImageBufs& w, BlockBatch& bt, const BlockBatchDev& dev)
{
    const size_t cnt = bt.count();
    int err;
    // ---- raw blocks: the chunks' bytes straight into the image, behind the BlockIndex ----
    bt.r_first.clear(), bt.r_count.clear(), bt.r_payload.clear();
    uint64_t raw_bytes = 0;
    for (size_t i = 0; i < cnt; ++i)
        if (bt.codec[i].codec == LTHIP_CODEC_NONE && bt.place[i] != PLACE_IN_IMAGE)
        {
            const uint32_t nchunks = bt.first[i + 1] - bt.first[i];
            bt.r_first.push_back(dev.chunk_base + bt.first[i]);
            bt.r_count.push_back(nchunks);
            bt.r_payload.push_back(bt.img_off[i] + lthip_block_index_size(nchunks));
            raw_bytes += bt.raw[i];
        }
    if (!bt.r_first.empty() &&
        (err = lthip_raw_copy_blocks(ctx, (uint32_t)bt.r_first.size(), bt.r_first.data(), bt.r_count.data(), bt.r_payload.data(), dev.chunk_base,
                                     bt.first[cnt], dev.d_lens, dev.d_raw_offsets, dev.d_raw_src, dev.d_arena, raw_bytes + 1)))
        return err;
    // ---- the codec, straight to image + header size: the keys in the order they appear, and per key the places in theirs ----
    for (const BlockCodec& key : bt.keys)
        for (uint32_t place = 0; place < dev.nplaces; ++place)
        {
            bt.c_src.clear(), bt.c_size.clear(), bt.c_dst.clear(), bt.c_cap.clear(), bt.which.clear();
            for (size_t i = 0; i < cnt; ++i)
                if (bt.place[i] == place && bt.codec[i] == key)
                {
                    bt.c_src.push_back(bt.src_off[i]);
                    bt.c_size.push_back(bt.raw[i]);
                    bt.c_dst.push_back(bt.img_off[i] + lthip_stored_block_header_size(bt.first[i + 1] - bt.first[i]));
                    bt.c_cap.push_back((uint32_t)block_codec_bound(key.codec, bt.raw[i]));
                    bt.which.push_back((uint32_t)i);
                }
            if (bt.which.empty())
                continue;
            // the codec entry points write one size per block of the call: a run of neighbours writes them in place, anything else goes
            // through a list of the call's own and is scattered by `which` (the gather kernel on 4-byte ranges)
            const uint32_t k = (uint32_t)bt.which.size();
            bool contiguous = true;
            for (uint32_t i = 1; i < k; ++i)
                contiguous &= bt.which[i] == bt.which[i - 1] + 1;
            uint32_t* d_sizes = dev.d_comp + bt.which[0];
            if (!contiguous)
            {
                if ((err = reserve_dev(ctx, w.d_tmpsz, (size_t)k * 4)))
                    return err;
                d_sizes = (uint32_t*)w.d_tmpsz.p;
            }
            if (key.codec == LTHIP_CODEC_LZ4)
                err = lthip_lz4_compress_blocks(ctx, dev.places[place], k, bt.c_src.data(), bt.c_size.data(), dev.d_arena, bt.c_dst.data(),
                                                bt.c_cap.data(), d_sizes, 0);
            else
                err = lthip_zstd_compress_blocks_q(ctx, dev.places[place], k, bt.c_src.data(), bt.c_size.data(), dev.d_arena, bt.c_dst.data(),
                                                   bt.c_cap.data(), d_sizes, key.quality);
            if (err)
                return err;
            if (!contiguous)
            {
                bt.scatter.clear();
                for (uint32_t i = 0; i < k; ++i)
                    bt.scatter.add((uint64_t)i * 4u, 4u, (uint64_t)bt.which[i] * 4u, 0);
                if ((err = lthip_gather_upload(ctx, w, w.d_tmpsz.p, bt.scatter, dev.d_comp)))
                    return err;
            }
        }
    return 0;
}

int lthip_block_headers_upload(lthip_ctx* ctx, BlockImageBufs& w, const BlockBatch& bt, bool with_tags)
{
    const size_t cnt = bt.count();
    hipStream_t s = ctx->stream;
    int err;
    if ((err = reserve_dev(ctx, w.d_bfirst, (cnt + 1) * 4)) || (err = reserve_dev(ctx, w.d_braw, cnt * 4)) ||
        (err = reserve_dev(ctx, w.d_bimg, cnt * 8)) || (err = reserve_dev(ctx, w.d_btag, cnt * 4)) ||
        (err = lthip_stage_upload(ctx, w.d_bfirst.p, bt.first.data(), (cnt + 1) * 4, s)) ||
        (err = lthip_stage_upload(ctx, w.d_braw.p, bt.raw.data(), cnt * 4, s)) ||
        (err = lthip_stage_upload(ctx, w.d_bimg.p, bt.img_off.data(), cnt * 8, s)))
        return err;
    return with_tags ? lthip_stage_upload(ctx, w.d_btag.p, bt.tag.data(), cnt * 4, s) : 0;
}

int lthip_block_headers(lthip_ctx* ctx, const BlockImageBufs& w, const BlockBatch& bt, const BlockBatchDev& dev, const lthip_ingest_config& cfg,
                        bool with_tags)
{
    // (tag 0 means a raw image only where the session writes by tag -- a raw block gets the BlockIndex alone, and its entry of d_comp is
    // filled in with its raw size; LTHIP_CODEC_LZ4 / _ZSTD compress a tag-0 block like any other)
    const uint32_t raw_mode = cfg.codec == LTHIP_CODEC_NONE || cfg.codec == LTHIP_CODEC_BY_TAG ? 1u : 0u;
    return lthip_launch_block_headers(ctx, LTHIP_K_OTHER, (const uint32_t*)w.d_bfirst.p, (uint32_t)bt.count(), dev.d_hashes + dev.chunk_base,
                                      dev.d_lens + dev.chunk_base, dev.d_bhash, cfg.hash_identifier, cfg.compression_type,
                                      with_tags ? (const uint32_t*)w.d_btag.p : nullptr, (const uint32_t*)w.d_braw.p, dev.d_comp,
                                      (const uint64_t*)w.d_bimg.p, dev.d_arena, raw_mode);
}
