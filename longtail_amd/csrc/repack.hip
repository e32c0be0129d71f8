// repack.hip -- the repack session (include/longtail_hip.h, "the repack session"): the live chunks of a store's under-used blocks out of
// their blocks and into new stored-block images, on the device and from the blocks themselves.  What the reference answers with
// Longtail_GetExistingStoreIndex(.., min_block_usage_percent) + Longtail_CreateMissingContent + Longtail_WriteContent over the source
// files, for a store keeper who has the blocks and not the files.
//
//   create   which blocks stay is lthip_get_existing_store_index, byte for byte; what the new blocks are is
//            lthip_create_missing_content over the moved chunks: the index side is those two calls, not a restatement of their rules.
//            The device plans what lies between them.  The StoreIndex's chunk hashes go into an lthip_seen (a hash's first position:
//            its SOURCE block is the first block in StoreIndex order that holds it), the kept blocks' chunk hashes into a second, the
//            live list into a third (first occurrences).  k_repack_resolve gives every live hash its size, its source block's tag and
//            whether it moves -- first occurrence, held by the store, held by no kept block --, a scan of those flags and
//            k_repack_compact make the moved list in the live list's order.  With the new index on the host, repack_plan.h lays the
//            work buffer out and k_repack_dest (a wave per new block) turns the block bases into a destination per moved chunk.
//            (moved hash, length, destination) is an occurrence list: the restore session takes it as it takes a VersionIndex's
//            (lthip_restore_create_occurrences), and its plan, check, decode, verify and scatter are the ones every restore runs.
//   blocks   lthip_restore_blocks of that session, with the work buffer as its output.
//   write    the ingest sessions' block writer (block_images.hip) over the new blocks: a tagged block is compressed from its staged
//            range straight into its image, a tag-0 block's chunks lie in its image already (PLACE_IN_IMAGE: nothing is copied), then
//            BlockIndex and [raw][compressed] words around them.  The block hashes are the new index's.
//   finish   the restore session's finish, with the compressed sizes on their way to the host in front of its wait.
#include "ingest_buffers.h"
#include "lthip_internal.h"
#include "repack_plan.h"
#include "restore_plan.h"

namespace
{

using restore_plan::NONE;

// what the plan's kernels count for the host
struct Counters
{
    unsigned long long unknown;     // live hashes the StoreIndex does not hold
    unsigned long long live;        // distinct live hashes
    unsigned long long moved_bytes; // bytes of the moved chunks
};

struct StoreTabs
{
    const uint32_t *csize, *cblock, *btag; // per chunk position its size and block, per block its tag
};

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1)
        v += __shfl_xor(v, o, 64);
    return v;
}

// per live hash i: pos[i] its first position in the StoreIndex's chunk list (NONE: unknown), kpos[i] its position among the kept blocks'
// chunks (NONE: no kept block holds it), first[i] the first position of its hash in the live list.  moves[i] = 1: it is moved.
__global__ void k_repack_resolve(uint32_t n, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ kpos, const uint32_t* __restrict__ first,
                                 StoreTabs sv, uint32_t* __restrict__ moves, uint32_t* __restrict__ len, uint32_t* __restrict__ tag,
                                 Counters* counters)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool unknown = false, distinct = false;
    unsigned long long bytes = 0;
    if (i < n)
    {
        const uint32_t p = pos[i];
        const uint32_t b = p == NONE ? NONE : sv.cblock[p];
        distinct = first[i] == i;
        unknown = b == NONE;
        const bool mv = distinct && !unknown && kpos[i] == NONE;
        const uint32_t l = unknown ? 0u : sv.csize[p];
        moves[i] = mv ? 1u : 0u;
        len[i] = l;
        tag[i] = unknown ? 0u : sv.btag[b];
        bytes = mv ? l : 0u;
    }
    const uint64_t mu = __builtin_amdgcn_ballot_w64(unknown), md = __builtin_amdgcn_ballot_w64(distinct);
    bytes = wave_sum(bytes);
    if ((threadIdx.x & 63) == 0)
    {
        if (mu)
            atomicAdd(&counters->unknown, (unsigned long long)__builtin_popcountll(mu));
        if (md)
            atomicAdd(&counters->live, (unsigned long long)__builtin_popcountll(md));
        if (bytes)
            atomicAdd(&counters->moved_bytes, bytes);
    }
}

// the moved list in the live list's order: rank = the exclusive scan of moves
__global__ void k_repack_compact(uint32_t n, const uint64_t* __restrict__ live, const uint32_t* __restrict__ moves, const uint32_t* __restrict__ rank,
                                 const uint32_t* __restrict__ len, const uint32_t* __restrict__ tag, uint64_t* __restrict__ m_hash,
                                 uint32_t* __restrict__ m_len, uint32_t* __restrict__ m_tag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !moves[i])
        return;
    const uint32_t k = rank[i];
    m_hash[k] = live[i];
    m_len[k] = len[i];
    m_tag[k] = tag[i];
}

// One wave per new block: block b holds moved chunks [bfirst[b], bfirst[b + 1]), the first goes to byte bdest[b] of the work buffer and
// the others follow it back to back -- an exclusive scan of the block's chunk sizes, 64 chunks a round (a block's sizes sum below 2^32).
__global__ __launch_bounds__(64) void k_repack_dest(const uint32_t* __restrict__ bfirst, uint32_t nblocks, const uint64_t* __restrict__ bdest,
                                                    const uint32_t* __restrict__ len, uint64_t* __restrict__ dst)
{
    const uint32_t b = blockIdx.x;
    if (b >= nblocks)
        return;
    const uint32_t lane = threadIdx.x, c0 = bfirst[b], n = bfirst[b + 1] - c0;
    uint64_t run = bdest[b];
    for (uint32_t base = 0; base < n; base += 64) // (wave-uniform bounds: every lane takes part in the shuffles)
    {
        const uint32_t i = base + lane;
        const uint32_t v = i < n ? len[c0 + i] : 0u;
        uint32_t inc = v;
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t t = __shfl_up(inc, d, 64);
            if ((int)lane >= d)
                inc += t;
        }
        if (i < n)
            dst[c0 + i] = run + (inc - v);
        run += __shfl(inc, 63, 64);
    }
}

int upload(lthip_ctx* ctx, void* d_dst, const void* h_src, size_t bytes)
{
    constexpr size_t PIECE = 4u << 20;
    for (size_t o = 0; o < bytes; o += PIECE)
        if (const int err = lthip_stage_upload(ctx, (uint8_t*)d_dst + o, (const uint8_t*)h_src + o, std::min(PIECE, bytes - o), ctx->stream))
            return err;
    return 0;
}
template <class T> int upload(lthip_ctx* ctx, DBuf& d, const std::vector<T>& h)
{
    const int err = reserve_dev(ctx, d, h.size() * sizeof(T));
    return err ? err : upload(ctx, d.p, h.data(), h.size() * sizeof(T));
}

template <class K, class... A> int launch(lthip_ctx* ctx, K kernel, dim3 grid, dim3 block, A... args)
{
    LaunchTimer tm(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, args...);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

uint64_t bound_of_tag(uint32_t tag, uint32_t raw) { return block_codec_bound((uint32_t)codec_of_tag(tag), raw); }

// an lthip_seen that destroys itself
struct SeenHolder
{
    lthip_seen* t = nullptr;
    ~SeenHolder() { lthip_seen_destroy(t); }
};

} // namespace

struct lthip_repack
{
    lthip_ctx* ctx = nullptr;
    uint32_t percent = 0, max_block_size = 0, max_chunks = 0, verify = 0, hash_identifier = 0;
    std::vector<uint8_t> kept_index, new_index, after_index; // serialized: get_existing's, create_missing_content's, kept merged with new
    std::vector<uint64_t> kept, dropped, source;             // block hashes: kept in the kept index's order, the others in the store's
    repack_plan::Layout lay;
    lthip_repack_info info = {};
    lthip_restore* rs = nullptr; // the moved chunks as a restore session whose output is the work buffer
    DBuf d_mhash, d_mlen, d_bhash, d_comp; // moved chunks (= the new index's chunk list), per new block its hash and payload size
    BlockImageBufs wbufs;
    BlockBatch bt;
    std::vector<uint32_t> comp, image_sizes;
    const void* d_work = nullptr; // the work buffer of the first call that was given one
    bool written = false, done = false, bad = false;
};

extern "C" void lthip_repack_destroy(lthip_repack* p)
{
    if (!p)
        return;
    (void)hipSetDevice(p->ctx->device);
    lthip_restore_destroy(p->rs); // (waits for what was queued)
    (void)hipStreamSynchronize(p->ctx->stream);
    delete p;
}

static int repack_build(lthip_repack* p, const void* store_index, size_t size, uint64_t live_count, const uint64_t* d_live)
{
    lthip_ctx* ctx = p->ctx;
    const char* const who = "lthip_repack_create";
    restore_parse::StoreIndex si, ki, ni;
    if (restore_parse::parse_store_index(store_index, size, &si))
        return lthip_fail(ctx, EBADF, who, "malformed store index");
    if (live_count > 0x7FFFFFF0ull)
        return lthip_fail(ctx, EINVAL, who, "more than 2^31 live hashes");
    p->hash_identifier = si.hash_identifier;
    const char* why = "";
    int err, refused;
    // ---- kept: lthip_get_existing_store_index, as it is (a subset of the store's blocks: the store index's size holds it) ----
    size_t got = 0;
    p->kept_index.resize(std::max<size_t>(size, 16));
    if ((err = lthip_get_existing_store_index(ctx, store_index, size, live_count, d_live, p->percent, p->kept_index.data(), p->kept_index.size(), &got)))
        return err;
    p->kept_index.resize(got);
    if (restore_parse::parse_store_index(p->kept_index.data(), got, &ki))
        return lthip_fail(ctx, EIO, who, "the kept index does not parse");
    std::vector<uint8_t> is_kept;
    repack_plan::block_lists(si, ki, &is_kept);
    for (uint32_t i = 0; i < ki.block_count; ++i)
        p->kept.push_back(ki.block_hashes[i]);
    for (uint32_t b = 0; b < si.block_count; ++b)
        if (!is_kept[b])
            p->dropped.push_back(si.block_hashes[b]);
    // ---- the host tables of the store, and the kept blocks' chunk hashes (the `existing` of lthip_create_missing_content) ----
    restore_plan::StoreTables st;
    if ((refused = restore_plan::store_tables(si, &st, &why)))
        return lthip_fail(ctx, refused, who, why);
    const uint32_t m = si.chunk_count, km = ki.chunk_count, n = (uint32_t)live_count;
    std::vector<uint64_t> kchash(km);
    for (uint32_t c = 0; c < km; ++c)
        kchash[c] = ki.chunk_hashes[c];
    // ---- the plan on the device ----
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DBuf d_chash, d_csize, d_cblock, d_btag, d_kchash, d_sfirst, d_kfirst, d_pos, d_kpos, d_first, d_moves, d_rank, d_len, d_tag, d_mtag, d_counters;
    if ((err = upload(ctx, d_chash, st.chash)) || (err = upload(ctx, d_csize, st.csize)) || (err = upload(ctx, d_cblock, st.cblock)) ||
        (err = upload(ctx, d_btag, st.btag)) || (err = upload(ctx, d_kchash, kchash)))
        return err;
    if ((err = reserve_dev(ctx, d_sfirst, (size_t)m * 4)) || (err = reserve_dev(ctx, d_kfirst, (size_t)km * 4)) || (err = reserve_dev(ctx, d_pos, (size_t)n * 4)) ||
        (err = reserve_dev(ctx, d_kpos, (size_t)n * 4)) || (err = reserve_dev(ctx, d_first, (size_t)n * 4)) || (err = reserve_dev(ctx, d_moves, (size_t)n * 4)) ||
        (err = reserve_dev(ctx, d_rank, ((size_t)n + 1) * 4)) || (err = reserve_dev(ctx, d_len, (size_t)n * 4)) || (err = reserve_dev(ctx, d_tag, (size_t)n * 4)) ||
        (err = reserve_dev(ctx, d_mtag, (size_t)n * 4)) || (err = reserve_dev(ctx, d_counters, sizeof(Counters))) ||
        (err = reserve_dev(ctx, p->d_mhash, (size_t)n * 8)) || (err = reserve_dev(ctx, p->d_mlen, (size_t)n * 4)))
        return err;
    LTHIP_CHECK(ctx, hipMemsetAsync(d_counters.p, 0, sizeof(Counters), s));
    LTHIP_CHECK(ctx, hipMemsetAsync(d_rank.p, 0, ((size_t)n + 1) * 4, s));
    Counters counters = {};
    uint32_t moved = 0;
    std::vector<uint32_t> mtag;
    {
        SeenHolder seen_store, seen_kept, seen_live;
        if ((err = lthip_seen_create(ctx, m, &seen_store.t)) || (err = lthip_seen_add(seen_store.t, m, (const uint64_t*)d_chash.p, (uint32_t*)d_sfirst.p, nullptr)) ||
            (err = lthip_seen_create(ctx, km, &seen_kept.t)) || (err = lthip_seen_add(seen_kept.t, km, (const uint64_t*)d_kchash.p, (uint32_t*)d_kfirst.p, nullptr)) ||
            (err = lthip_seen_create(ctx, n, &seen_live.t)) || (err = lthip_seen_add(seen_live.t, n, d_live, (uint32_t*)d_first.p, nullptr)))
            return err;
        if (n)
        {
            const StoreTabs sv = {(const uint32_t*)d_csize.p, (const uint32_t*)d_cblock.p, (const uint32_t*)d_btag.p};
            const dim3 grid((n + 255u) / 256u), block(256);
            if ((err = lthip_seen_find(seen_store.t, n, d_live, (uint32_t*)d_pos.p)) || (err = lthip_seen_find(seen_kept.t, n, d_live, (uint32_t*)d_kpos.p)) ||
                (err = launch(ctx, k_repack_resolve, grid, block, n, (const uint32_t*)d_pos.p, (const uint32_t*)d_kpos.p, (const uint32_t*)d_first.p, sv,
                              (uint32_t*)d_moves.p, (uint32_t*)d_len.p, (uint32_t*)d_tag.p, (Counters*)d_counters.p)) ||
                (err = lthip_exclusive_scan_u32(ctx, (const uint32_t*)d_moves.p, (uint32_t*)d_rank.p, n, nullptr, LTHIP_K_OTHER)) ||
                (err = launch(ctx, k_repack_compact, grid, block, n, d_live, (const uint32_t*)d_moves.p, (const uint32_t*)d_rank.p, (const uint32_t*)d_len.p,
                              (const uint32_t*)d_tag.p, (uint64_t*)p->d_mhash.p, (uint32_t*)p->d_mlen.p, (uint32_t*)d_mtag.p)))
                return err;
        }
        // ---- the plan's read-back: the counters, how many chunks move, their tags (lthip_create_missing_content takes tags from the host) ----
        mtag.resize(n);
        LTHIP_CHECK(ctx, hipMemcpyAsync(&counters, d_counters.p, sizeof counters, hipMemcpyDeviceToHost, s));
        LTHIP_CHECK(ctx, hipMemcpyAsync(&moved, (const uint32_t*)d_rank.p + n, 4, hipMemcpyDeviceToHost, s));
        if (n)
            LTHIP_CHECK(ctx, hipMemcpyAsync(mtag.data(), d_mtag.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    }
    if (counters.unknown)
        return lthip_fail(ctx, ENOENT, who, "the live list names a chunk hash the store index does not hold");
    for (uint32_t k = 0; k < moved; ++k)
        if (codec_of_tag(mtag[k]) < 0)
            return lthip_fail(ctx, ENOTSUP, who, "a source block's tag names no codec of this library");
    // ---- new: lthip_create_missing_content over the moved chunks, as it is ----
    p->new_index.resize(store_index_size(moved, moved));
    if ((err = lthip_create_missing_content(ctx, km, (const uint64_t*)d_kchash.p, moved, (const uint64_t*)p->d_mhash.p, (const uint32_t*)p->d_mlen.p, mtag.data(),
                                            si.hash_identifier, p->max_block_size, p->max_chunks, p->new_index.data(), p->new_index.size(), &got)))
        return err;
    p->new_index.resize(got);
    if (restore_parse::parse_store_index(p->new_index.data(), got, &ni) || ni.chunk_count != moved)
        return lthip_fail(ctx, EIO, who, "the new index does not list the moved chunks");
    if ((refused = repack_plan::layout(ni, bound_of_tag, &p->lay, &why)))
        return lthip_fail(ctx, refused, who, why);
    const repack_plan::Layout& lay = p->lay;
    const uint32_t nnb = ni.block_count;
    // ---- destinations: the block bases from the layout, the chunks of a block back to back behind them ----
    DBuf d_bfirst, d_bdest, d_dst;
    std::vector<uint64_t> bhash(nnb);
    for (uint32_t b = 0; b < nnb; ++b)
        bhash[b] = ni.block_hashes[b];
    if ((err = upload(ctx, d_bfirst, lay.first)) || (err = upload(ctx, d_bdest, lay.dest)) || (err = upload(ctx, p->d_bhash, bhash)) ||
        (err = reserve_dev(ctx, p->d_comp, (size_t)nnb * 4)) || (err = reserve_dev(ctx, d_dst, (size_t)moved * 8)))
        return err;
    if (nnb && (err = launch(ctx, k_repack_dest, dim3(nnb), dim3(64), (const uint32_t*)d_bfirst.p, nnb, (const uint64_t*)d_bdest.p, (const uint32_t*)p->d_mlen.p,
                             (uint64_t*)d_dst.p)))
        return err;
    // ---- the moved chunks as a restore session: its plan, and its one wait (the tables above are read until then) ----
    const lthip_restore_config rcfg = {sizeof(lthip_restore_config), p->verify};
    const lthip_occurrence_list list = {si.hash_identifier, moved, (const uint64_t*)p->d_mhash.p, (const uint32_t*)p->d_mlen.p, (const uint64_t*)d_dst.p};
    if ((err = lthip_restore_create_occurrences(ctx, &rcfg, &list, store_index, size, lay.work_bytes, who, &p->rs)))
        return err;
    uint64_t ns = 0;
    (void)lthip_restore_needed_blocks(p->rs, nullptr, 0, &ns);
    p->source.resize((size_t)ns);
    (void)lthip_restore_needed_blocks(p->rs, p->source.data(), ns, &ns);
    // ---- the store index afterwards: the kept blocks under their own tags, then the new blocks ----
    std::vector<uint8_t> kept_own = p->kept_index;
    repack_plan::own_tags(si, ki, kept_own.data());
    size_t asize = 0;
    refused = lthip_store_index_merge(kept_own.data(), kept_own.size(), p->new_index.data(), p->new_index.size(), nullptr, 0, &asize);
    if (refused != ENOMEM && refused != 0)
        return lthip_fail(ctx, refused, who, "the kept and the new index do not merge");
    p->after_index.resize(asize);
    if ((refused = lthip_store_index_merge(kept_own.data(), kept_own.size(), p->new_index.data(), p->new_index.size(), p->after_index.data(), asize, &asize)))
        return lthip_fail(ctx, refused, who, "the kept and the new index do not merge");
    lthip_repack_info& f = p->info;
    f.blocks_total = si.block_count, f.blocks_kept = p->kept.size(), f.blocks_dropped = p->dropped.size(), f.blocks_source = p->source.size();
    f.live_chunks = counters.live, f.moved_chunks = moved, f.moved_bytes = counters.moved_bytes, f.new_blocks = nnb;
    f.staging_bytes = lay.staging_bytes, f.work_bytes = lay.work_bytes;
    f.kept_index_size = p->kept_index.size(), f.new_index_size = p->new_index.size(), f.store_index_size = p->after_index.size();
    return 0;
}

extern "C" int lthip_repack_create(lthip_ctx* ctx, const lthip_repack_config* cfg, const void* store_index, size_t store_index_size,
                                   uint64_t live_count, const uint64_t* d_live_hashes, lthip_repack** out)
{
    if (out)
        *out = nullptr;
    if (!ctx || !cfg || !store_index || !out || (live_count && !d_live_hashes))
        return EINVAL;
    if (cfg->struct_size < 20 || cfg->struct_size > 4096)
        return lthip_fail(ctx, EINVAL, "lthip_repack_create", "config->struct_size must be set to sizeof(lthip_repack_config)");
    if (cfg->min_block_usage_percent > 100)
        return lthip_fail(ctx, EINVAL, "lthip_repack_create", "min_block_usage_percent above 100");
    if (!cfg->max_block_size || !cfg->max_chunks_per_block)
        return lthip_fail(ctx, EINVAL, "lthip_repack_create", "max_block_size and max_chunks_per_block must not be 0");
    lthip_repack* p = new (std::nothrow) lthip_repack();
    if (!p)
        return ENOMEM;
    p->ctx = ctx;
    p->percent = cfg->min_block_usage_percent, p->max_block_size = cfg->max_block_size, p->max_chunks = cfg->max_chunks_per_block;
    p->verify = cfg->struct_size >= 24 && cfg->verify ? 1u : 0u;
    const int err = lthip_guarded(ctx, "lthip_repack_create", [&] { return repack_build(p, store_index, store_index_size, live_count, d_live_hashes); });
    if (err)
    {
        lthip_repack_destroy(p); // (waits for what was queued; nothing stays allocated)
        return err;
    }
    *out = p;
    return 0;
}

extern "C" int lthip_repack_plan_info(const lthip_repack* p, lthip_repack_info* out)
{
    if (!p || !out || out->struct_size < 16 || out->struct_size > 4096)
        return EINVAL;
    lthip_repack_info f = p->info;
    f.struct_size = std::min<uint64_t>(out->struct_size, sizeof f);
    memcpy(out, &f, (size_t)f.struct_size);
    return 0;
}

static int hash_list(const std::vector<uint64_t>& list, uint64_t* hashes, uint64_t capacity, uint64_t* count)
{
    if (!count)
        return EINVAL;
    *count = list.size();
    if (hashes && capacity >= list.size() && !list.empty())
        memcpy(hashes, list.data(), list.size() * 8);
    return 0;
}
extern "C" int lthip_repack_kept_blocks(const lthip_repack* p, uint64_t* hashes, uint64_t capacity, uint64_t* count)
{
    return p ? hash_list(p->kept, hashes, capacity, count) : EINVAL;
}
extern "C" int lthip_repack_dropped_blocks(const lthip_repack* p, uint64_t* hashes, uint64_t capacity, uint64_t* count)
{
    return p ? hash_list(p->dropped, hashes, capacity, count) : EINVAL;
}
extern "C" int lthip_repack_source_blocks(const lthip_repack* p, uint64_t* hashes, uint64_t capacity, uint64_t* count)
{
    return p ? hash_list(p->source, hashes, capacity, count) : EINVAL;
}

static int blob_out(const std::vector<uint8_t>& blob, void* out, size_t capacity, size_t* size)
{
    if (!size)
        return EINVAL;
    *size = blob.size();
    if (!out || capacity < blob.size())
        return ENOMEM;
    memcpy(out, blob.data(), blob.size());
    return 0;
}
extern "C" int lthip_repack_kept_index(const lthip_repack* p, void* out, size_t capacity, size_t* size)
{
    return p ? blob_out(p->kept_index, out, capacity, size) : EINVAL;
}

extern "C" size_t lthip_repack_scratch_bound(const lthip_repack* p, uint32_t block_count, const uint64_t* block_hashes)
{
    return p ? lthip_restore_scratch_bound(p->rs, block_count, block_hashes) : 0;
}

extern "C" int lthip_repack_blocks(lthip_repack* p, uint32_t block_count, const uint64_t* block_hashes, const void* d_images, const uint64_t* image_offsets,
                                   const uint32_t* image_sizes, void* d_scratch, uint64_t scratch_bytes, void* d_work)
{
    if (!p)
        return EINVAL;
    if (p->bad)
        return lthip_fail(p->ctx, EBADF, "lthip_repack_blocks", "a delivered block was bad: the session is over");
    if (p->written)
        return lthip_fail(p->ctx, EEXIST, "lthip_repack_blocks", "the images were written");
    if ((uintptr_t)d_work & 7u)
        return lthip_fail(p->ctx, EINVAL, "lthip_repack_blocks", "the work buffer must be 8-byte aligned");
    if (p->d_work && d_work && d_work != p->d_work)
        return lthip_fail(p->ctx, EINVAL, "lthip_repack_blocks", "another work buffer than the one before");
    const int err = lthip_restore_blocks(p->rs, block_count, block_hashes, d_images, image_offsets, image_sizes, d_scratch, scratch_bytes, d_work);
    if (!err && d_work)
        p->d_work = d_work;
    return err;
}

static int repack_write(lthip_repack* p, void* d_work)
{
    lthip_ctx* ctx = p->ctx;
    const repack_plan::Layout& lay = p->lay;
    const uint32_t nnb = (uint32_t)lay.raw.size();
    lthip_ingest_config icfg;
    memset(&icfg, 0, sizeof icfg);
    icfg.hash_identifier = p->hash_identifier;
    icfg.codec = LTHIP_CODEC_BY_TAG;
    BlockBatch& bt = p->bt;
    bt.clear();
    for (uint32_t b = 0; b < nnb; ++b)
    {
        const uint32_t tag = lay.tag[b];
        bt.add(lay.first[b + 1] - lay.first[b], lay.raw[b], tag, block_codec(icfg, tag), tag ? 0u : PLACE_IN_IMAGE, tag ? lay.stage[b] : 0u);
        bt.img_off[b] = lay.image[b]; // (the session's own layout, repack_plan.h: the staging region lies in front of the images)
    }
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    const BlockBatchDev dev = {{d_work, nullptr, nullptr}, 1, (const uint64_t*)p->d_mhash.p, (const uint32_t*)p->d_mlen.p, 0u, nullptr, nullptr,
                               (const uint64_t*)p->d_bhash.p, (uint32_t*)p->d_comp.p, d_work};
    int err;
    if ((err = lthip_block_payloads(ctx, p->wbufs, bt, dev)) || (err = lthip_block_headers_upload(ctx, p->wbufs, bt, true)))
        return err;
    return lthip_block_headers(ctx, p->wbufs, bt, dev, icfg, true);
}

extern "C" int lthip_repack_write(lthip_repack* p, void* d_work, uint64_t work_bytes)
{
    if (!p)
        return EINVAL;
    lthip_ctx* ctx = p->ctx;
    if ((uintptr_t)d_work & 7u)
        return lthip_fail(ctx, EINVAL, "lthip_repack_write", "the work buffer must be 8-byte aligned");
    if (p->bad)
        return lthip_fail(ctx, EBADF, "lthip_repack_write", "a delivered block was bad: the session is over");
    if (p->written)
        return lthip_fail(ctx, EEXIST, "lthip_repack_write", "the images were written before");
    if (lthip_restore_outstanding(p->rs))
        return lthip_fail(ctx, ENOENT, "lthip_repack_write", "source blocks are outstanding");
    if (p->info.new_blocks)
    {
        if (!d_work || (p->d_work && d_work != p->d_work))
            return lthip_fail(ctx, EINVAL, "lthip_repack_write", "null work buffer, or another one than the blocks calls were given");
        if (work_bytes < p->info.work_bytes)
            return lthip_fail(ctx, ENOMEM, "lthip_repack_write", "work buffer below info.work_bytes");
        const int err = lthip_guarded(ctx, "lthip_repack_write", [&] { return repack_write(p, d_work); });
        if (err)
            return err;
    }
    p->written = true;
    return 0;
}

extern "C" int lthip_repack_finish(lthip_repack* p, void* h_new_index, size_t capacity, size_t* out_size, lthip_repack_result* out)
{
    if (!p || (out && (out->struct_size < 16 || out->struct_size > 4096)))
        return EINVAL;
    lthip_ctx* ctx = p->ctx;
    const uint32_t nnb = (uint32_t)p->info.new_blocks;
    int code = lthip_guarded(ctx, "lthip_repack_finish", [&] { return p->comp.resize(nnb), 0; });
    if (code)
        return code;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (p->written && nnb) // (in front of the restore session's wait)
        LTHIP_CHECK(ctx, hipMemcpyAsync(p->comp.data(), p->d_comp.p, (size_t)nnb * 4, hipMemcpyDeviceToHost, ctx->stream));
    lthip_restore_result rr;
    memset(&rr, 0, sizeof rr);
    rr.struct_size = sizeof rr;
    code = lthip_restore_finish(p->rs, &rr);
    if (code == EBADF)
        p->bad = true;
    else if (code == 0 && !p->written)
        code = ENOENT; // every source block is there: lthip_repack_write is outstanding
    lthip_repack_result res;
    memset(&res, 0, sizeof res);
    res.blocks_source = rr.blocks_needed;
    res.blocks_delivered = rr.blocks_delivered;
    res.blocks_bad = rr.blocks_bad;
    res.chunks_mismatched = rr.chunks_mismatched;
    res.decoded_bytes = rr.decoded_bytes;
    if (code == 0)
    {
        if ((code = lthip_guarded(ctx, "lthip_repack_finish", [&] { return p->image_sizes.resize(nnb), 0; })))
            return code;
        for (uint32_t b = 0; b < nnb; ++b)
        {
            if (p->lay.tag[b] && !p->comp[b])
                return lthip_fail(ctx, EIO, "lthip_repack_finish", "an encoder returned no payload");
            p->image_sizes[b] = (uint32_t)repack_plan::header_bytes(p->lay.first[b + 1] - p->lay.first[b], p->lay.tag[b]) + p->comp[b];
            res.raw_bytes_written += p->lay.raw[b];
            res.compressed_bytes_written += p->comp[b];
        }
        p->done = true;
    }
    if (out)
    {
        res.struct_size = std::min<uint64_t>(out->struct_size, sizeof res);
        memcpy(out, &res, (size_t)res.struct_size);
    }
    if (out_size)
        *out_size = p->new_index.size();
    if (code == 0 && h_new_index)
    {
        if (capacity < p->new_index.size())
            return ENOMEM;
        memcpy(h_new_index, p->new_index.data(), p->new_index.size());
    }
    return code;
}

extern "C" int lthip_repack_images(const lthip_repack* p, uint64_t* count, const uint64_t** offsets, const uint32_t** sizes)
{
    if (!p || !count)
        return EINVAL;
    if (p->bad)
        return lthip_fail(p->ctx, EBADF, "lthip_repack_images", "a delivered block was bad: no image is handed out");
    if (!p->done)
        return lthip_fail(p->ctx, EINVAL, "lthip_repack_images", "valid after lthip_repack_finish returned 0");
    *count = p->lay.image.size();
    if (offsets)
        *offsets = p->lay.image.data();
    if (sizes)
        *sizes = p->image_sizes.data();
    return 0;
}

extern "C" int lthip_repack_store_index(const lthip_repack* p, void* out, size_t capacity, size_t* size)
{
    if (!p || !size)
        return EINVAL;
    if (p->bad)
        return lthip_fail(p->ctx, EBADF, "lthip_repack_store_index", "a delivered block was bad: the store stays as it is");
    if (!p->done)
        return lthip_fail(p->ctx, EINVAL, "lthip_repack_store_index", "valid after lthip_repack_finish returned 0");
    return blob_out(p->after_index, out, capacity, size);
}

extern "C" int lthip_repack_block_status(const lthip_repack* p, uint32_t count, const uint64_t* block_hashes, uint32_t* status)
{
    return p ? lthip_restore_block_status(p->rs, count, block_hashes, status) : EINVAL;
}
