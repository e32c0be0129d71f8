// ingest_stream.hip -- the ingest session for a tree that arrives in SLICES (include/longtail_hip.h): contiguous runs of jobs, chunked
// and hashed by the caller slice after slice, and still ONE VersionIndex / StoreIndex pair and the reference's packing of the whole
// tree at the end.
//
//   first-seen      one lthip_seen table for the session (k_dedup.hip): a chunk is written if it is new in its slice's lthip_seen_add
//   the store       with an lthip_store attached (lthip_ingest_stream_set_store) a new chunk is written only if the store lacks it:
//                   lthip_store_find over the slice's hashes beside the first-seen pass, a byte per chunk to the host with the lists.
//                   Everything behind the unique list -- packing, carry, assembly, codec -- runs over the shorter list unchanged
//   packing         Longtail_CreateStoreIndex's greedy rule (src/longtail.c:6801-6860) over the unique list of the whole tree, continued
//                   from slice to slice: a block is closed only when the chunk that does not fit any more has been seen.  At the end of
//                   a slice one block may be open; its chunk list stays on the host, its BYTES are gathered into d_carry
//   assembly        a block that is one byte range of the slice (or of d_carry) is compressed where it lies, every other one is
//                   gathered first -- the carried bytes from d_carry, the slice's chunks from d_data (lthip_gather_ranges)
//   indexes         the host keeps hash and length of every chunk (12 bytes per chunk, pinned), the unique list and the block table;
//                   finish builds the VersionIndex with lthip_build_version_index over the kept lists and writes the StoreIndex from
//                   its own block table
//
// A slice call waits once, for the slice's lists (24 bytes per chunk) to reach the host: the packing is serial, in the reference too.
// It does not wait for the codec: what the codec and the hash of a call produce for the host (block hashes, compressed sizes) lands in
// a pinned batch record and is collected by lthip_ingest_stream_images, by finish, or by a later call once its event has fired.
// The passes of different slices are NOT overlapped here: everything is queued on the context's one stream.
#include "lthip_internal.h"
#include "ingest_buffers.h"

#include <algorithm>

struct lthip_ingest_stream
{
    lthip_ctx* ctx = nullptr;
    lthip_ingest_config cfg = {};
    // ---- the tree (deep copy) ----
    uint32_t na = 0;
    std::vector<uint64_t> asset_sizes;
    std::vector<uint32_t> path_offsets;
    std::vector<uint16_t> permissions;
    std::vector<char> path_data;
    std::vector<uint32_t> tags; // per asset: the caller's, or cfg.compression_type
    uint64_t njobs = 0;
    std::vector<uint32_t> job_asset;
    std::vector<uint64_t> job_size;
    std::vector<uint32_t> asset_chunks; // chunks of every asset so far
    // ---- state ----
    lthip_seen* seen = nullptr;
    const lthip_store* store = nullptr;                          // what the target already holds (may be null): its chunks are not written
    uint64_t unique_all = 0, known_chunks = 0, known_bytes = 0; // the version's distinct chunks so far; those of them the store held
    uint64_t next_job = 0;
    bool started = false; // a slice call has begun work: the store can no longer be attached or detached
    bool closed = false;  // finish has closed the open block: no more slices
    int sticky = 0;       // a failure after work had started: what every later call returns
    // ---- every chunk of the tree so far: hash and length (pinned: the slices' lists are copied straight into them) ----
    HBuf h_all_hash, h_all_len;
    uint64_t n_all = 0;
    // ---- the unique list and the blocks it is packed into ----
    std::vector<uint64_t> u_hash;
    std::vector<uint32_t> u_len, u_tag;
    std::vector<uint64_t> b_first{0}; // nb + 1 indices into the unique list
    std::vector<uint64_t> b_size;
    std::vector<uint32_t> b_tag;
    std::vector<uint64_t> b_hash; // collected from the batch records (blocks [0, b_hash.size()))
    std::vector<uint32_t> b_comp;
    uint64_t gathered_blocks = 0, gathered_bytes = 0;
    // ---- the open block: chunks [b_first.back(), u_len.size()), their bytes back to back in d_carry ----
    DBuf d_carry;
    std::vector<uint64_t> carry_off;
    uint64_t carry_bytes = 0;
    // ---- per call ----
    HBuf h_first, h_off, h_pf, h_known;
    DBuf d_known;
    DBuf d_usrc; // raw blocks: the address of every chunk of the call (d_carry or the slice's data)
    DBuf d_first, d_gather, d_uh, d_ul, d_boff, d_blen, d_bhash, d_comp;
    BlockImageBufs wbufs; // the block writer's tables (block_images.hip)
    DBuf d_vh, d_vl; // finish: the kept lists on the device
    std::vector<uint64_t> u_src; // byte offset in the slice's data of the chunks this slice added to the unique list
    Event ev_lists, ev_call;
    // what a call's launches produce for the host: [nb u64 block hashes][nb u32 compressed sizes], behind an event
    struct Batch
    {
        HBuf h;
        uint64_t nb = 0;
        Event ev;
    };
    std::vector<Batch> pending, spare;
    // ---- the blocks of the call being written (kept for its vectors), and the images of the last call ----
    BlockBatch batch;
    BlockImages img;
};

namespace
{

typedef lthip_ingest_stream Stream;

uint64_t block_limit(const lthip_ingest_config* cfg) { return block_limit(cfg->max_block_size); }

bool config_ok(const lthip_ingest_config* cfg)
{
    // (a block is one codec call's source: below the codecs' 2^31 - 2^25 bytes)
    return cfg && cfg->max_block_size != 0 && cfg->max_block_size <= 0x70000000u && cfg->max_chunks_per_block != 0 &&
           cfg->codec <= LTHIP_CODEC_BY_TAG;
}

int stream_fail(Stream* s, int err)
{
    if (err)
        s->sticky = err;
    return err;
}

// The batch records whose work has run (wait: all of them) into b_hash / b_comp, in block order.
int stream_collect(Stream* s, bool wait)
{
    lthip_ctx* ctx = s->ctx;
    size_t done = 0;
    for (; done < s->pending.size(); ++done)
    {
        Stream::Batch& b = s->pending[done];
        if (wait)
            LTHIP_CHECK(ctx, hipEventSynchronize(b.ev));
        else
        {
            const hipError_t e = hipEventQuery(b.ev);
            if (e == hipErrorNotReady)
                break;
            LTHIP_CHECK(ctx, e);
        }
        const uint64_t* hashes = (const uint64_t*)b.h.p;
        const uint32_t* comp = (const uint32_t*)((const uint8_t*)b.h.p + b.nb * 8);
        s->b_hash.insert(s->b_hash.end(), hashes, hashes + b.nb);
        s->b_comp.insert(s->b_comp.end(), comp, comp + b.nb);
        s->spare.push_back(std::move(b));
    }
    s->pending.erase(s->pending.begin(), s->pending.begin() + done);
    return 0;
}

// Greedy packing of the unique list (Longtail_CreateStoreIndex :6801-6860), continued from the open block.  Unless `final`, a block is
// only closed when the chunk that does not fit any more has been seen, or when it holds max_chunks_per_block chunks.
void stream_pack(Stream* s, bool final)
{
    const uint64_t nu = s->u_len.size(), limit = block_limit(&s->cfg), max_chunks = s->cfg.max_chunks_per_block;
    uint64_t i = s->b_first.back();
    while (i < nu)
    {
        uint64_t size;
        const uint64_t j = next_block_end(s->u_len.data(), s->u_tag.data(), i, nu, max_chunks, limit, &size);
        if (j == nu && !final && j - i < max_chunks)
            break; // the next chunk may still belong to this block
        s->b_size.push_back(size);
        s->b_first.push_back(j);
        s->b_tag.push_back(s->u_tag[i]);
        i = j;
    }
}

// gathers merge neighbours up to this many bytes (Ranges::add): the open block is usually one byte range of the slice, up to
// max_block_size * 1.1, and still spreads over the device
constexpr uint64_t MERGE_BYTES = 128u << 10;

// The images of blocks [b0, b1) into the arena: assembly, codec, block hashes, BlockIndex + [raw][compressed] around the payloads
// (:4111-4150; compressblockstore.c:103-139).  Chunks below `fresh` (an index into the unique list) lie in d_carry at carry_off, the others
// in d_data at u_src.  A block's codec follows cfg.codec and its tag (block_codec): a raw block is copied from where its chunks lie, the
// others are compressed with one call per (codec, quality, place).
int stream_emit(Stream* s, size_t b0, size_t b1, const void* d_data, uint64_t fresh, void* d_arena, uint64_t arena_bytes)
{
    lthip_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    BlockBatch& bt = s->batch;
    bt.clear();
    s->img.set(b0, bt);
    const size_t cnt = b1 - b0;
    if (!cnt)
        return 0;
    const uint64_t c0 = s->b_first[b0], c1 = s->b_first[b1], nc = c1 - c0, open0 = fresh - s->carry_off.size();
    int err;
    // ---- where every block's bytes are: place 0 in d_data, 1 to be gathered, 2 in d_carry; a raw block is copied chunk run by chunk
    // run from wherever they are: its chunks' addresses (the two places are two allocations: the copy takes them relative to a null base) ----
    std::vector<uint64_t> addr;
    Ranges from_carry, from_data;
    uint64_t pos = 0;
    for (size_t b = b0; b < b1; ++b)
    {
        const uint64_t first = s->b_first[b], last = s->b_first[b + 1];
        const BlockCodec bc = block_codec(s->cfg, s->b_tag[b]);
        uint32_t place = 1;
        uint64_t off = 0;
        if (bc.codec == LTHIP_CODEC_NONE)
        {
            place = PLACE_RAW;
            addr.resize(nc, 0);
            for (uint64_t c = first; c < last; ++c)
                addr[c - c0] = c < fresh ? (uint64_t)(uintptr_t)s->d_carry.p + s->carry_off[c - open0] : (uint64_t)(uintptr_t)d_data + s->u_src[c - fresh];
        }
        else if (last <= fresh) // (carried chunks lie back to back)
        {
            place = 2;
            off = s->carry_off[first - open0];
        }
        else if (first >= fresh)
        {
            place = 0;
            off = s->u_src[first - fresh];
            for (uint64_t c = first + 1; c < last && place == 0; ++c)
                if (s->u_src[c - fresh] != s->u_src[c - 1 - fresh] + s->u_len[c - 1])
                    place = 1;
        }
        if (place == 1)
        {
            off = pos = (pos + 15u) & ~(uint64_t)15u;
            for (uint64_t c = first; c < last; ++c)
            {
                if (c < fresh)
                    from_carry.add(s->carry_off[c - open0], s->u_len[c], pos, MERGE_BYTES);
                else
                    from_data.add(s->u_src[c - fresh], s->u_len[c], pos, MERGE_BYTES);
                pos += s->u_len[c];
            }
            ++s->gathered_blocks;
            s->gathered_bytes += s->b_size[b];
        }
        bt.add((uint32_t)(last - first), s->b_size[b], s->b_tag[b], bc, place, off);
    }
    if (bt.arena > arena_bytes) // (lthip_ingest_stream_arena_bound is a bound of this sum: tests/test_ingest_stream_abi.py)
        return lthip_fail(ctx, ENOMEM, "lthip_ingest_stream", "the arena does not hold the call's images");
    if ((err = reserve_dev(ctx, s->d_comp, cnt * 4)) || (err = reserve_dev(ctx, s->d_bhash, cnt * 8)) || (err = reserve_dev(ctx, s->d_boff, cnt * 8)) ||
        (err = reserve_dev(ctx, s->d_blen, cnt * 4)) || (err = reserve_dev(ctx, s->d_uh, nc * 8)) || (err = reserve_dev(ctx, s->d_ul, nc * 4)))
        return err;
    // ---- block assembly (WriteContentBlockJob, :4640-4721) for the blocks that are not one byte range ----
    if (pos && ((err = reserve_dev(ctx, s->d_gather, pos + 256)) || (err = lthip_gather_upload(ctx, s->wbufs, s->d_carry.p, from_carry, s->d_gather.p)) ||
                (err = lthip_gather_upload(ctx, s->wbufs, d_data, from_data, s->d_gather.p))))
        return err;
    // ---- the chunk lengths of the call's blocks (the raw copy and the BlockIndex kernel read them), the raw blocks' addresses ----
    if ((err = lthip_stage_upload(ctx, s->d_ul.p, s->u_len.data() + c0, nc * 4, st)))
        return err;
    if (!addr.empty() && ((err = reserve_dev(ctx, s->d_usrc, nc * 8)) || (err = lthip_stage_upload(ctx, s->d_usrc.p, addr.data(), nc * 8, st))))
        return err;
    const BlockBatchDev dev = {{d_data, s->d_gather.p, s->d_carry.p}, 3, (const uint64_t*)s->d_uh.p, (const uint32_t*)s->d_ul.p, 0u,
                               (const uint64_t*)s->d_usrc.p, nullptr, (const uint64_t*)s->d_bhash.p, (uint32_t*)s->d_comp.p, d_arena};
    if ((err = lthip_block_payloads(ctx, s->wbufs, bt, dev)))
        return err;
    // ---- block hashes = hash of each block's chunk-hash array (:3753-3757), then the bytes around the payloads (always with the blocks' tags) ----
    BlockHashRanges r;
    r.fill(bt.first.data(), cnt, 0);
    if ((err = lthip_stage_upload(ctx, s->d_uh.p, s->u_hash.data() + c0, nc * 8, st)) ||
        (err = lthip_stage_upload(ctx, s->d_boff.p, r.off.data(), cnt * 8, st)) || (err = lthip_stage_upload(ctx, s->d_blen.p, r.len.data(), cnt * 4, st)) ||
        (err = lthip_block_headers_upload(ctx, s->wbufs, bt, true)) ||
        (err = lthip_hash_ranges_by_id(ctx, s->cfg.hash_identifier, s->d_uh.p, cnt, (const uint64_t*)s->d_boff.p, (const uint32_t*)s->d_blen.p, r.max_len,
                                       r.leaves, (uint64_t*)s->d_bhash.p)) ||
        (err = lthip_block_headers(ctx, s->wbufs, bt, dev, s->cfg, true)))
        return err;
    // ---- block hashes and compressed sizes on their way to the host ----
    if (s->spare.empty())
    {
        Stream::Batch fresh;
        LTHIP_CHECK(ctx, fresh.ev.create());
        s->spare.push_back(std::move(fresh));
    }
    if ((err = reserve_pinned(ctx, s->spare.back().h, cnt * 12)))
        return err;
    s->pending.push_back(std::move(s->spare.back()));
    s->spare.pop_back();
    Stream::Batch& rec = s->pending.back();
    rec.nb = cnt;
    LTHIP_CHECK(ctx, hipMemcpyAsync(rec.h.p, s->d_bhash.p, cnt * 8, hipMemcpyDeviceToHost, st));
    LTHIP_CHECK(ctx, hipMemcpyAsync((uint8_t*)rec.h.p + cnt * 8, s->d_comp.p, cnt * 4, hipMemcpyDeviceToHost, st));
    LTHIP_CHECK(ctx, hipEventRecord(rec.ev, st));
    s->img.set(b0, bt);
    return 0;
}

// room for `chunks` more entries in the kept lists; the entries so far move (every copy into the old buffers has been waited for)
int stream_grow_lists(Stream* s, uint64_t chunks)
{
    lthip_ctx* ctx = s->ctx;
    const uint64_t want = s->n_all + chunks;
    if (s->h_all_hash.cap >= want * 8 && s->h_all_len.cap >= want * 4)
        return 0;
    const uint64_t cap = std::max<uint64_t>(want, 2 * s->n_all);
    HBuf nh, nl;
    int err;
    if ((err = reserve_pinned(ctx, nh, cap * 8)) || (err = reserve_pinned(ctx, nl, cap * 4)))
        return err;
    if (s->n_all)
    {
        memcpy(nh.p, s->h_all_hash.p, s->n_all * 8);
        memcpy(nl.p, s->h_all_len.p, s->n_all * 4);
    }
    s->h_all_hash = std::move(nh); // (the old lists leave with nh / nl)
    s->h_all_len = std::move(nl);
    return 0;
}

int stream_slice_work(Stream* s, uint64_t first_job, uint64_t job_count, uint64_t slice_bytes, const void* d_data, const uint64_t* d_offs,
                      const uint32_t* d_lens, const uint64_t* d_hashes, const uint32_t* d_part_first, uint64_t chunks, void* d_arena,
                      uint64_t arena_bytes)
{
    lthip_ctx* ctx = s->ctx;
    hipStream_t st = ctx->stream;
    int err;
    if ((err = stream_collect(s, false)))
        return err;
    if ((err = reserve_pinned(ctx, s->h_first, chunks * 4)) || (err = reserve_pinned(ctx, s->h_off, chunks * 8)) ||
        (err = reserve_pinned(ctx, s->h_pf, (job_count + 1) * 4)) || (err = reserve_dev(ctx, s->d_first, chunks * 4)) ||
        (err = stream_grow_lists(s, chunks)))
        return err;
    if (s->store && ((err = reserve_pinned(ctx, s->h_known, chunks)) || (err = reserve_dev(ctx, s->d_known, chunks))))
        return err;
    // ---- first-seen over everything so far, then the slice's lists to the host: the call's one wait ----
    const uint64_t base = s->n_all;
    uint64_t* all_hash = (uint64_t*)s->h_all_hash.p + base;
    uint32_t* all_len = (uint32_t*)s->h_all_len.p + base;
    if (chunks)
    {
        if ((err = lthip_seen_add(s->seen, chunks, d_hashes, (uint32_t*)s->d_first.p, nullptr)))
            return err;
        if (s->store)
        {
            if ((err = lthip_store_find(s->store, chunks, d_hashes, (uint8_t*)s->d_known.p, nullptr)))
                return err;
            LTHIP_CHECK(ctx, hipMemcpyAsync(s->h_known.p, s->d_known.p, chunks, hipMemcpyDeviceToHost, st));
        }
        LTHIP_CHECK(ctx, hipMemcpyAsync(s->h_first.p, s->d_first.p, chunks * 4, hipMemcpyDeviceToHost, st));
        LTHIP_CHECK(ctx, hipMemcpyAsync(all_len, d_lens, chunks * 4, hipMemcpyDeviceToHost, st));
        LTHIP_CHECK(ctx, hipMemcpyAsync(all_hash, d_hashes, chunks * 8, hipMemcpyDeviceToHost, st));
        LTHIP_CHECK(ctx, hipMemcpyAsync(s->h_off.p, d_offs, chunks * 8, hipMemcpyDeviceToHost, st));
        LTHIP_CHECK(ctx, hipMemcpyAsync(s->h_pf.p, d_part_first, (job_count + 1) * 4, hipMemcpyDeviceToHost, st));
        LTHIP_CHECK(ctx, hipEventRecord(s->ev_lists, st));
        LTHIP_CHECK(ctx, hipEventSynchronize(s->ev_lists));
    }
    else
        memset(s->h_pf.p, 0, (job_count + 1) * 4);
    const uint32_t* first = (const uint32_t*)s->h_first.p;
    const uint64_t* offs = (const uint64_t*)s->h_off.p;
    const uint32_t* pf = (const uint32_t*)s->h_pf.p;
    const uint8_t* known = s->store ? (const uint8_t*)s->h_known.p : nullptr;
    if (pf[0] != 0 || pf[job_count] != chunks)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_slice", "d_part_first does not span the slice's chunks");
    uint64_t sum = 0;
    for (uint64_t j = 0; j < chunks; ++j)
        sum += all_len[j];
    if (sum != slice_bytes) // (the arena was sized from the jobs' bytes)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_slice", "the chunk lengths do not add up to the bytes of these jobs");
    for (uint64_t j = 0; j < chunks; ++j)
        if (all_len[j] > block_limit(&s->cfg)) // (lists of a chunker with a larger maximum than create assumed: d_carry and the arena bound hold a block)
            return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_slice", "a chunk is larger than max_block_size * 1.1");
    // ---- the chunks that are new (and that the store lacks): onto the unique list, with their asset's tag ----
    const uint64_t fresh = s->u_len.size();
    s->u_src.clear();
    for (uint64_t m = 0; m < job_count; ++m)
    {
        if (pf[m + 1] < pf[m] || pf[m + 1] > chunks)
            return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_slice", "d_part_first is not ascending");
        const uint32_t a = s->job_asset[first_job + m], tag = s->tags[a];
        s->asset_chunks[a] += pf[m + 1] - pf[m];
        for (uint64_t j = pf[m]; j < pf[m + 1]; ++j)
            if (first[j] == (uint32_t)(base + j))
            {
                ++s->unique_all;
                if (known && known[j])
                {
                    ++s->known_chunks;
                    s->known_bytes += all_len[j];
                    continue;
                }
                s->u_hash.push_back(all_hash[j]);
                s->u_len.push_back(all_len[j]);
                s->u_tag.push_back(tag);
                s->u_src.push_back(offs[j]);
            }
    }
    s->n_all += chunks;
    s->next_job += job_count;
    // ---- the blocks this slice closes, then the bytes of the block it leaves open ----
    const size_t b0 = s->b_size.size();
    stream_pack(s, false);
    const size_t b1 = s->b_size.size();
    if ((err = stream_emit(s, b0, b1, d_data, fresh, d_arena, arena_bytes)))
        return err;
    if (b1 > b0) // (the first block closed took every carried chunk with it: the open block is all of this slice)
    {
        s->carry_off.clear();
        s->carry_bytes = 0;
    }
    Ranges keep;
    for (uint64_t c = std::max<uint64_t>(s->b_first.back(), fresh); c < s->u_len.size(); ++c)
    {
        keep.add(s->u_src[c - fresh], s->u_len[c], s->carry_bytes, MERGE_BYTES);
        s->carry_off.push_back(s->carry_bytes);
        s->carry_bytes += s->u_len[c];
    }
    if (s->carry_bytes > block_limit(&s->cfg))
        return lthip_fail(ctx, EIO, "lthip_ingest_stream_slice", "the open block outgrew a block");
    if ((err = lthip_gather_upload(ctx, s->wbufs, d_data, keep, s->d_carry.p)))
        return err;
    LTHIP_CHECK(ctx, hipEventRecord(s->ev_call, st));
    return 0;
}

} // namespace

extern "C" size_t lthip_ingest_stream_arena_bound(const lthip_ingest_config* cfg, uint64_t slice_bytes, uint64_t slice_chunks)
{
    if (!config_ok(cfg))
        return 0;
    // A call closes blocks of at most R = slice_bytes + L bytes in N = slice_chunks + max_chunks_per_block chunks (L: the largest block, the
    // block carried in).  With bound(a) + bound(b) <= bound(a + b) + bound(0) for both codecs -- their bounds are n + floor(n / k) + c(n),
    // c(n) <= c(0) -- and at most N blocks of sum(n_b) <= N chunks:
    //   sum round64(header(n_b) + bound(raw_b)) <= bound(R) + N * (header(0) + bound(0) + 63) + 12 * N
    // LTHIP_CODEC_NONE: a slot is round64(lthip_block_index_size(n_b) + raw_b), the same sum with bound(n) = n and the BlockIndex for the
    // header.  LTHIP_CODEC_BY_TAG: a block takes one of the three, so a slot is at most the largest of the three,
    // round64(header(n_b) + m(raw_b)) with m(n) = n + floor(n / 255) + 64 >= each codec's bound (zstd's is n + (n >> 8) + at most 64, LZ4's
    // n + floor(n / 255) + 16), and m(a) + m(b) <= m(a + b) + m(0) again: the same sum with m for the bound.  That is no less than the
    // bound of any one codec.
    const uint64_t R = slice_bytes + block_limit(cfg), N = slice_chunks + cfg->max_chunks_per_block;
    auto of = [&](uint32_t codec) -> size_t {
        const size_t per_chunk = block_header_bytes(codec, 1) + block_codec_bound(codec, 0) + 63u;
        const size_t whole = codec == LTHIP_CODEC_ZSTD   ? lthip_zstd_bound((size_t)R)
                             : codec == LTHIP_CODEC_LZ4  ? (size_t)(R + R / 255 + 16) // (lthip_lz4_bound stops at 2^31)
                                                         : (size_t)R;
        return whole + (size_t)N * per_chunk;
    };
    if (cfg->codec != LTHIP_CODEC_BY_TAG)
        return of(cfg->codec);
    return (size_t)(R + R / 255 + 64) + (size_t)N * (lthip_stored_block_header_size(1) + 64u + 63u);
}

// Every buffer and event of the session frees itself (ingest_buffers.h): nothing goes before the stream that may touch it is idle.
extern "C" void lthip_ingest_stream_destroy(lthip_ingest_stream* s)
{
    if (!s)
        return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    lthip_seen_destroy(s->seen);
    delete s;
}

extern "C" int lthip_ingest_stream_create(lthip_ctx* ctx, const lthip_ingest_config* cfg, const lthip_ingest_tree* t, lthip_ingest_stream** out)
{
    if (!ctx || !cfg || !t || !out)
        return EINVAL;
    *out = nullptr;
    if (!config_ok(cfg))
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_create", "bad block / codec parameters");
    if (t->my_jobs)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_create", "my_jobs must be NULL: the stream session is single-GPU");
    // The open block waits in a buffer of L = max_block_size * 1.1 bytes, and the arena bound counts L carried bytes.  A chunk above L
    // would be a block of its own in the reference; here it is refused up front: the largest chunk of the reference's chunker is
    // max(48, 2 * target_chunk_size) (src/longtail.c:1985-1987).
    if (std::max<uint64_t>(48, 2ull * cfg->target_chunk_size) > block_limit(cfg))
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_create", "2 * target_chunk_size must not exceed max_block_size * 1.1");
    if ((t->job_count && !t->job_asset) || (t->asset_count && (!t->asset_sizes || !t->path_start_offsets || !t->permissions || !t->path_data)))
        return EINVAL;
    // every tag the tree carries must be one the codec mode writes (include/longtail_hip.h, TAGS AND CODECS)
    // (cfg.compression_type too, as lthip_ingest_create checks it: it is the tag of every asset when there are no asset tags)
    for (uint32_t a = 0; a < (t->asset_tags ? t->asset_count + 1u : 1u); ++a)
        if (const int refused = tag_refusal(cfg->codec, a ? t->asset_tags[a - 1] : cfg->compression_type))
            return lthip_fail(ctx, refused, "lthip_ingest_stream_create", tag_refusal_text(refused));
    // the jobs of lthip_make_jobs: asset after asset, 1 + size / part jobs each (src/longtail.c:2399-2404, 2432-2457)
    const uint32_t na = t->asset_count;
    const uint64_t part = (uint64_t)cfg->target_chunk_size * 1024u;
    std::vector<uint64_t> job_size(t->job_count);
    uint64_t j = 0, tree_bytes = 0;
    for (uint32_t a = 0; a < na; ++a)
    {
        if (t->path_start_offsets[a] >= t->path_data_size)
            return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_create", "path offset outside the path data");
        const uint64_t size = t->asset_sizes[a], jobs = part ? 1 + size / part : 1;
        tree_bytes += size;
        for (uint64_t k = 0; k < jobs; ++k, ++j)
        {
            if (j >= t->job_count || t->job_asset[j] != a)
                return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_create", "the job table is not lthip_make_jobs' of these assets");
            job_size[j] = std::min(part, size - k * part);
        }
    }
    if (j != t->job_count)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_create", "the job table is not lthip_make_jobs' of these assets");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    lthip_ingest_stream* s = new (std::nothrow) lthip_ingest_stream();
    if (!s)
        return ENOMEM;
    s->ctx = ctx;
    s->cfg = *cfg;
    s->na = na;
    s->asset_sizes.assign(t->asset_sizes, t->asset_sizes + na);
    s->path_offsets.assign(t->path_start_offsets, t->path_start_offsets + na);
    s->permissions.assign(t->permissions, t->permissions + na);
    s->path_data.assign(t->path_data, t->path_data + t->path_data_size);
    if (t->asset_tags)
        s->tags.assign(t->asset_tags, t->asset_tags + na);
    else
        s->tags.assign(na, cfg->compression_type); // one tag for the whole tree (what UpSync passes, cmd/main.c:1038-1046)
    s->njobs = t->job_count;
    s->job_asset.assign(t->job_asset, t->job_asset + t->job_count);
    s->job_size.swap(job_size);
    s->asset_chunks.assign(na, 0);
    // the lists and the table for the chunks the tree is expected to come to (chunks average the target size or more); both grow
    const uint64_t expect = std::min<uint64_t>(cfg->target_chunk_size ? tree_bytes / cfg->target_chunk_size + t->job_count : t->job_count, 1ull << 28);
    int err = 0;
    if (s->ev_lists.create() != hipSuccess || s->ev_call.create() != hipSuccess)
        err = lthip_fail(ctx, EIO, "lthip_ingest_stream_create", "hipEventCreate");
    if (!err)
        err = lthip_seen_create(ctx, expect, &s->seen);
    if (!err)
        err = reserve_dev(ctx, s->d_carry, block_limit(cfg) + 256);
    if (!err)
        err = stream_grow_lists(s, expect);
    if (err)
    {
        lthip_ingest_stream_destroy(s);
        return err;
    }
    *out = s;
    return 0;
}

extern "C" uint64_t lthip_ingest_stream_table_grown(const lthip_ingest_stream* s) { return s ? lthip_seen_grown(s->seen) : 0; }

extern "C" int lthip_ingest_stream_set_store(lthip_ingest_stream* s, const lthip_store* store)
{
    if (!s)
        return EINVAL;
    if (s->sticky)
        return s->sticky;
    // (refused before any work: the session stays as it is)
    if (s->started || s->closed)
        return lthip_fail(s->ctx, EINVAL, "lthip_ingest_stream_set_store", "the store is attached before the first slice");
    if (store && lthip_store_ctx(store) != s->ctx)
        return lthip_fail(s->ctx, EINVAL, "lthip_ingest_stream_set_store", "the store belongs to another context");
    s->store = store;
    return 0;
}

extern "C" int lthip_ingest_stream_store_stats(const lthip_ingest_stream* s, uint64_t* known_chunks, uint64_t* known_bytes)
{
    if (!s)
        return EINVAL;
    if (known_chunks)
        *known_chunks = s->known_chunks;
    if (known_bytes)
        *known_bytes = s->known_bytes;
    return 0;
}

extern "C" int lthip_ingest_stream_slice(lthip_ingest_stream* s, uint64_t first_job, uint64_t job_count, const void* d_data,
                                         const uint64_t* d_chunk_offsets, const uint32_t* d_chunk_lens, const uint64_t* d_chunk_hashes,
                                         const uint32_t* d_part_first, uint64_t chunks, void* d_arena, uint64_t arena_bytes)
{
    if (!s)
        return EINVAL;
    lthip_ctx* ctx = s->ctx;
    if (s->sticky)
        return s->sticky;
    // ---- refused before any work: the session stays as it is ----
    if (s->closed)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_slice", "the session is finished");
    if (first_job != s->next_job || job_count > s->njobs - first_job)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_slice", "slices are contiguous runs of jobs in job order");
    if (chunks && (!d_data || !d_chunk_offsets || !d_chunk_lens || !d_chunk_hashes || !d_part_first || !d_arena))
        return EINVAL;
    if (s->n_all + chunks > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_slice", "more than 2^31 - 1 chunks");
    uint64_t bytes = 0;
    for (uint64_t m = 0; m < job_count; ++m)
        bytes += s->job_size[first_job + m];
    if (arena_bytes < lthip_ingest_stream_arena_bound(&s->cfg, bytes, chunks))
        return lthip_fail(ctx, ENOMEM, "lthip_ingest_stream_slice", "arena below lthip_ingest_stream_arena_bound of this slice");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    s->started = true;
    return stream_fail(s, stream_slice_work(s, first_job, job_count, bytes, d_data, d_chunk_offsets, d_chunk_lens, d_chunk_hashes, d_part_first,
                                            chunks, d_arena, arena_bytes));
}

extern "C" int lthip_ingest_stream_images(lthip_ingest_stream* s, uint64_t* out_first_block, uint64_t* out_count, const uint64_t** out_offsets,
                                          const uint32_t** out_sizes)
{
    if (!s)
        return EINVAL;
    if (s->sticky)
        return s->sticky;
    lthip_ctx* ctx = s->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    int err = stream_collect(s, true);
    if (!err && hipEventSynchronize(s->ev_call) != hipSuccess) // (the open block's bytes are in d_carry: the caller's buffers are its own again)
        err = lthip_fail(ctx, EIO, "lthip_ingest_stream_images", "hipEventSynchronize");
    if (err)
        return stream_fail(s, err);
    s->img.complete(s->b_comp.data());
    s->img.get(out_first_block, out_count, out_offsets, out_sizes);
    return 0;
}

extern "C" int lthip_ingest_stream_finish(lthip_ingest_stream* s, void* d_arena, uint64_t arena_bytes, void* h_version_index,
                                          size_t version_index_capacity, void* h_store_index, size_t store_index_capacity,
                                          lthip_ingest_result* out)
{
    if (!s)
        return EINVAL;
    lthip_ctx* ctx = s->ctx;
    if (s->sticky)
        return s->sticky;
    // ---- refused before any work ----
    if (!result_struct_ok(out))
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_finish", RESULT_STRUCT_TEXT);
    if (s->next_job != s->njobs)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_stream_finish", "not every job of the tree has been delivered");
    const bool open = s->b_first.back() < s->u_len.size();
    if (!s->closed && (arena_bytes < lthip_ingest_stream_arena_bound(&s->cfg, 0, 0) || (open && !d_arena)))
        return lthip_fail(ctx, ENOMEM, "lthip_ingest_stream_finish", "arena below lthip_ingest_stream_arena_bound(cfg, 0, 0)");
    const size_t nb = s->b_size.size() + (open ? 1 : 0), m = s->u_len.size();
    lthip_ingest_result res;
    memset(&res, 0, sizeof res);
    res.chunks_all = res.chunks_local = s->n_all;
    res.unique_all = s->unique_all;
    res.unique_local = m;
    res.blocks = nb;
    for (size_t c = 0; c < m; ++c)
        res.raw_bytes += s->u_len[c];
    res.version_index_size = lthip_version_index_size(s->na, s->unique_all, s->n_all, (uint32_t)s->path_data.size());
    res.store_index_size = store_index_size(nb, m);
    if ((h_version_index && version_index_capacity < res.version_index_size) || (h_store_index && store_index_capacity < res.store_index_size))
    {
        deliver_result(out, &res); // (both sizes; nothing done: the call may be repeated)
        return lthip_fail(ctx, ENOMEM, "lthip_ingest_stream_finish", "index buffer too small");
    }
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    int err = 0;
    if (!s->closed)
    {
        // ---- the open block: every chunk of it lies in d_carry ----
        const size_t b0 = s->b_size.size();
        stream_pack(s, true);
        s->closed = true;
        if ((err = stream_emit(s, b0, s->b_size.size(), nullptr, s->u_len.size(), d_arena, arena_bytes)))
            return stream_fail(s, err);
        if (hipEventRecord(s->ev_call, ctx->stream) != hipSuccess)
            return stream_fail(s, lthip_fail(ctx, EIO, "lthip_ingest_stream_finish", "hipEventRecord"));
    }
    if ((err = stream_collect(s, true)))
        return stream_fail(s, err);
    for (size_t b = 0; b < nb; ++b)
        res.compressed_bytes += s->b_comp[b];
    res.gathered_blocks = s->gathered_blocks;
    res.gathered_bytes = s->gathered_bytes;
    // ---- the VersionIndex of the whole tree over the kept lists (Longtail_CreateVersionIndex's tail) ----
    if (h_version_index)
    {
        const uint64_t n = s->n_all;
        if ((err = reserve_dev(ctx, s->d_vh, n * 8)) || (err = reserve_dev(ctx, s->d_vl, n * 4)))
            return stream_fail(s, err);
        if (n)
        {
            hipError_t e = hipMemcpyAsync(s->d_vh.p, s->h_all_hash.p, n * 8, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess)
                e = hipMemcpyAsync(s->d_vl.p, s->h_all_len.p, n * 4, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess)
                return stream_fail(s, lthip_fail(ctx, EIO, "lthip_ingest_stream_finish", hipGetErrorString(e)));
        }
        size_t size = 0;
        if ((err = lthip_build_version_index(ctx, s->na, s->asset_sizes.data(), s->path_offsets.data(), s->permissions.data(), s->path_data.data(),
                                             (uint32_t)s->path_data.size(), s->asset_chunks.data(), n, n ? (const uint64_t*)s->d_vh.p : nullptr,
                                             n ? (const uint32_t*)s->d_vl.p : nullptr, s->tags.data(), s->cfg.hash_identifier,
                                             s->cfg.target_chunk_size, h_version_index, version_index_capacity, &size)))
            return stream_fail(s, err);
        if (size != res.version_index_size)
            return stream_fail(s, lthip_fail(ctx, EIO, "lthip_ingest_stream_finish", "the VersionIndex's unique chunks are not the session's"));
    }
    // ---- the StoreIndex from the session's block table (Longtail_CreateStoreIndexFromBlocks :9060-9125, layout :8913-8931) ----
    if (h_store_index)
        write_store_index(h_store_index, s->cfg.hash_identifier, nb, m, s->b_hash.data(), s->u_hash.data(), s->b_first.data(), s->b_tag.data(), s->u_len.data());
    deliver_result(out, &res);
    return 0;
}
