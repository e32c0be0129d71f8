// ingest.hip -- the ingest metric of SURVEY.md §8(d) as ONE native session over device-resident assets:
//
//     Longtail_CreateVersionIndex   (src/longtail.c:2808)   chunk + hash (lthip_chunk_hash) -> [multi-GPU: exchange] ->
//                                                           first-seen dedup, content / path hashes, serialized VersionIndex
//     Longtail_CreateMissingContent (src/longtail.c:6882)   the chunks this rank saw first, packed into blocks
//                                                           (Longtail_CreateStoreIndex :6745-6880), block hashes, serialized StoreIndex
//     Longtail_WriteContent         (src/longtail.c:4760)   block assembly (device gather only where a block is not one byte
//                                                           range), per-block LZ4 / ZStd straight into the stored-block image,
//                                                           BlockIndex + [raw][compressed] around it (:4111-4150) -- a null sink:
//                                                           images are produced in a bounded device arena and dropped
//
// Everything between the phases stays on the device; the host sees the unique chunks' lengths and offsets once (the greedy
// packing is serial in the reference too) and does its serial work while the GPU is busy with work that does not depend on
// it: the VersionIndex sections are hashed and copied out while the host packs blocks, the StoreIndex is laid out while the
// codec runs.  No allocation in steady state: all workspaces are grown once and kept.
//
// Multi-GPU: the session is given ALL ranks' chunk hashes / lengths in job order (dist.exchange_chunks) plus
// the list of its own jobs.  Every rank derives the same first-seen table; a rank writes the chunks that are first-seen AND
// lie in its own jobs -- exactly Longtail_CreateMissingContent against a store that already holds the other ranks' chunks.
//
// A store that already has content (lthip_ingest_set_store): lthip_store_find over the rank's local chunks, and "this rank writes it"
// becomes first-seen, in its own jobs AND unknown to the store.  Everything behind that flag is as without a store.
#include "lthip_internal.h"
#include "index_kernels.h"
#include "ingest_buffers.h"

#include <algorithm>
#include <chrono>
#include <thread>

namespace
{

// local chunk k of this rank -> its index in the job-ordered arrays of all ranks.  part_first = the rank's own chunk-list starts
// (lthip_chunk_hash), one part per own job, job_gfirst[m] = index of own job m's first chunk in the global arrays.  With
// job_gfirst == null the arrays are the same.
__device__ __forceinline__ uint32_t ing_global_index(uint32_t k, const uint32_t* __restrict__ part_first, uint32_t nparts,
                                                     const uint32_t* __restrict__ job_gfirst)
{
    if (!job_gfirst)
        return k;
    uint32_t lo = 0, hi = nparts; // part m with part_first[m] <= k < part_first[m + 1] (empty parts: take the last such)
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (part_first[mid] <= k)
            lo = mid;
        else
            hi = mid;
    }
    return job_gfirst[lo] + (k - part_first[lo]);
}

// "this rank writes it": owned[k] = first_index[g(k)] == g(k), and -- with a store attached, known != null: lthip_store_find's flags
// of the local chunks -- the store does not hold it
__global__ void k_ing_owned(const uint32_t* __restrict__ first_index, const uint32_t* __restrict__ part_first, uint32_t nparts,
                            const uint32_t* __restrict__ job_gfirst, uint32_t nlocal, uint32_t* __restrict__ owned,
                            uint32_t* __restrict__ l2g, const uint8_t* __restrict__ known)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nlocal)
        return;
    const uint32_t g = ing_global_index(k, part_first, nparts, job_gfirst);
    l2g[k] = g;
    owned[k] = first_index[g] == g && !(known && known[k]) ? 1u : 0u;
}

// the hashes of a rank's local chunks out of the arrays of all ranks: what lthip_store_find is asked (multi-GPU only: for a single
// rank the arrays are the same)
__global__ void k_ing_local_hashes(const uint32_t* __restrict__ part_first, uint32_t nparts, const uint32_t* __restrict__ job_gfirst,
                                   uint32_t nlocal, const uint64_t* __restrict__ all_hashes, uint64_t* __restrict__ local_hashes)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nlocal)
        local_hashes[k] = all_hashes[ing_global_index(k, part_first, nparts, job_gfirst)];
}

// out[0] += first-seen local chunks the store holds, out[1] += their bytes (lthip_ingest_store_stats)
__global__ void k_ing_known_stats(const uint32_t* __restrict__ first_index, const uint32_t* __restrict__ l2g, const uint8_t* __restrict__ known,
                                  const uint32_t* __restrict__ all_lens, uint32_t nlocal, unsigned long long* __restrict__ out)
{
    unsigned long long chunks = 0, bytes = 0;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nlocal; k += gridDim.x * blockDim.x)
    {
        const uint32_t g = l2g[k];
        if (first_index[g] == g && known[k])
        {
            ++chunks;
            bytes += all_lens[g];
        }
    }
    for (int o = 32; o > 0; o >>= 1)
    {
        chunks += __shfl_down(chunks, o, 64);
        bytes += __shfl_down(bytes, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && chunks)
    {
        atomicAdd(out, chunks);
        atomicAdd(out + 1, bytes);
    }
}

// compaction of the owned chunks: hash, length, byte offset in the rank's data and the tag of the chunk's asset
__global__ void k_ing_compact(const uint32_t* __restrict__ owned, const uint32_t* __restrict__ orank, const uint32_t* __restrict__ l2g,
                              uint32_t nlocal, const uint64_t* __restrict__ all_hashes, const uint32_t* __restrict__ all_lens,
                              const uint64_t* __restrict__ local_offsets, const uint32_t* __restrict__ asset_first_chunk,
                              uint32_t asset_count, const uint32_t* __restrict__ asset_tags, uint64_t* __restrict__ u_hash,
                              uint32_t* __restrict__ u_len, uint64_t* __restrict__ u_off, uint32_t* __restrict__ u_tag)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nlocal || !owned[k])
        return;
    const uint32_t r = orank[k], g = l2g[k];
    u_hash[r] = all_hashes[g];
    u_len[r] = all_lens[g];
    u_off[r] = local_offsets[k];
    if (asset_tags)
    {
        uint32_t lo = 0, hi = asset_count;
        while (hi - lo > 1)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (asset_first_chunk[mid] <= g)
                lo = mid;
            else
                hi = mid;
        }
        u_tag[r] = asset_tags[lo];
    }
}

// brk[i] = chunk i does not continue the byte range of chunk i - 1 (what the packing loop needs of the offsets: a byte instead of 8)
__global__ void k_ing_breaks(const uint64_t* __restrict__ off, const uint32_t* __restrict__ len, uint32_t n, uint8_t* __restrict__ brk)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        brk[i] = i != 0u && off[i] != off[i - 1u] + len[i - 1u] ? 1 : 0;
}

__global__ void k_ing_sum_u32(const uint32_t* __restrict__ v, uint32_t n, unsigned long long* __restrict__ out)
{
    unsigned long long acc = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        acc += v[i];
    for (int o = 32; o > 0; o >>= 1)
        acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0 && acc)
        atomicAdd(out, acc);
}

} // namespace

// host tables of the job layout: the chunks of every asset and their exclusive sum (assets + 1), and for a rank of several the first
// chunk of each of its own jobs in the arrays of all ranks (own jobs + 1)
struct JobTables
{
    std::vector<uint32_t> starts, counts, gfirst;
};

// Every buffer and event frees itself (ingest_buffers.h); the initial values are stated here, once.
struct lthip_ingest
{
    lthip_ctx* ctx = nullptr;
    lthip_ingest_config cfg = {};
    // ---- index phase ----
    ViWorkspace vi; // the VersionIndex builder's tables (index_kernels.h); the owned chunks' compaction reads its d_starts / d_tags too
    DBuf d_first, d_counts;
    DBuf d_gfirst, d_owned, d_orank, d_l2g, d_mu_hash, d_mu_len, d_mu_off, d_mu_tag;
    // what the target already holds (lthip_ingest_set_store; may be null): the flags of the local chunks, and for a rank of several
    // their hashes
    const lthip_store* store = nullptr;
    DBuf d_known, d_lhash;
    uint64_t known_chunks = 0, known_bytes = 0;
    HBuf h_counts, h_mu_len, h_mu_off, h_mu_hash, h_mu_tag, h_bhash, h_comp, h_brk;
    DBuf d_brk;
    DBuf d_bhash, d_boff, d_blen, d_comp, d_sum;
    DBuf d_gather;
    BlockImageBufs wbufs; // the block writer's tables (block_images.hip)
    Event ev_counts, ev_lens, ev_offs, ev_index;
    // the first-seen index of every chunk computed elsewhere (the sharded table of the multi-GPU path): consumed by the next
    // lthip_ingest_index instead of its own table pass
    const uint32_t* ext_first = nullptr;
    uint64_t ext_unique = 0;
    // host state between the phases
    uint64_t n_all = 0, n_local = 0, unique_all = 0, n_mine = 0;
    std::vector<uint64_t> b_first;   // nb + 1 chunk indices into the owned-unique list
    std::vector<uint64_t> b_size;    // raw bytes
    std::vector<uint8_t> b_is_range; // the block's chunks are one byte range of the rank's data
    std::vector<uint32_t> b_tag;
    bool has_tags = false;
    size_t vi_size = 0;
    bool indexed = false, written = false;
    // the packing runs in slices (ingest_pack): lthip_ingest_index packs what the first codec batch takes, lthip_ingest_write the rest
    // once that batch is queued
    uint32_t pack_next = 0;   // first owned chunk that is in no block yet
    uint32_t pack_avail = 0;  // owned chunks whose lengths / break flags / tags / offsets are on the host
    uint64_t pack_raw = 0;    // raw bytes of the blocks so far
    bool blocks_done = false; // all blocks packed and hashed, their hashes on the way to the host (ev_index)
    Event ev_hashes;          // the owned chunks' hashes are on the host (side stream)
    lthip_ingest_result res = {};
    // the VersionIndex sections are put together by a helper thread on a context of its own (stream, staging ring, BLAKE3 scratch), so
    // that the calling thread keeps the session's context to itself and does not wait for it before lthip_ingest_finish
    lthip_ctx* vi_ctx = nullptr;
    std::thread vi_thread;
    int vi_err = 0;
    bool vi_pending = false; // prepared by lthip_ingest_index, not started yet
    // what the VersionIndex helper reads of the caller's tree AFTER lthip_ingest_index has returned: a deep copy (O(assets): sizes, path
    // offsets, permissions, path data, the job tables), so that a caller may free or reuse its lthip_ingest_tree arrays as soon as the call
    // returns -- the contract of round 2.  Only the device arrays and the output buffer live until lthip_ingest_finish (include/longtail_hip.h).
    ViTree vi_tree = {};
    std::vector<uint64_t> vi_asset_sizes;
    std::vector<uint32_t> vi_path_offsets;
    std::vector<uint16_t> vi_permissions;
    std::vector<char> vi_path_data;
    JobTables vi_jobs;
    const uint64_t* vi_hashes = nullptr;
    void* vi_out = nullptr;
    // the codec batch being written (kept for its vectors), and the stored-block images of the last one (lthip_ingest_images): their
    // sizes are completed by lthip_ingest_finish (they need the compressed sizes)
    BlockBatch batch;
    Ranges gather;
    BlockImages img;
};

// LTHIP_INGEST_TRACE=1: host time between the marks of lthip_ingest_index / _write, to stderr
struct IngTrace
{
    bool on;
    const char* what;
    std::chrono::steady_clock::time_point t0, last;
    char line[512];
    size_t len;
    explicit IngTrace(const char* w) : what(w), len(0)
    {
        LTHIP_ABLATION_ENV(env, "LTHIP_INGEST_TRACE");
        on = env.get() > 0;
        if (on)
            t0 = last = std::chrono::steady_clock::now();
    }
    void mark(const char* name)
    {
        if (!on)
            return;
        const auto now = std::chrono::steady_clock::now();
        if (len < sizeof line - 48)
            len += (size_t)snprintf(line + len, sizeof line - len, " %s %.0f", name, std::chrono::duration<double, std::micro>(now - last).count());
        last = now;
    }
    ~IngTrace()
    {
        if (on)
            fprintf(stderr, "%s (us):%s | total %.0f\n", what, line, std::chrono::duration<double, std::micro>(last - t0).count());
    }
};

extern "C" int lthip_ingest_create(lthip_ctx* ctx, const lthip_ingest_config* cfg, lthip_ingest** out)
{
    if (!ctx || !cfg || !out)
        return EINVAL;
    *out = nullptr;
    if (cfg->max_block_size == 0 || cfg->max_chunks_per_block == 0 || cfg->codec > LTHIP_CODEC_BY_TAG)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_create", "bad block / codec parameters");
    // (the tag of every block when lthip_ingest_index gets no asset tags; the asset tags are checked there)
    if (const int refused = tag_refusal(cfg->codec, cfg->compression_type))
        return lthip_fail(ctx, refused, "lthip_ingest_create", tag_refusal_text(refused));
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    lthip_ingest* g = new (std::nothrow) lthip_ingest();
    if (!g)
        return ENOMEM;
    g->ctx = ctx;
    g->cfg = *cfg;
    if (g->cfg.batch_bytes == 0)
        g->cfg.batch_bytes = 8ull << 30;
    for (Event* e : {&g->ev_counts, &g->ev_lens, &g->ev_offs, &g->ev_index, &g->ev_hashes})
        if (e->create() != hipSuccess)
        {
            lthip_ingest_destroy(g);
            return lthip_fail(ctx, EIO, "lthip_ingest_create", "hipEventCreate");
        }
    *out = g;
    return 0;
}

static int ingest_vi_join(lthip_ingest* g);

// Waits for what is in flight -- the helper thread with its context, the stream, the side stream's copies --, destroys what is not a
// buffer, and deletes: nothing is freed before the streams that may touch it are idle.
extern "C" void lthip_ingest_destroy(lthip_ingest* g)
{
    if (!g)
        return;
    (void)hipSetDevice(g->ctx->device);
    (void)ingest_vi_join(g);
    (void)hipStreamSynchronize(g->ctx->stream);
    if (g->ev_hashes)
        (void)hipEventSynchronize(g->ev_hashes);
    if (g->vi_ctx)
        lthip_ctx_destroy(g->vi_ctx);
    delete g;
}

// ---------------------------------------------------------------------------------------------------------------------
// phase 2: the tail of CreateVersionIndex + CreateMissingContent
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int lthip_ingest_set_first_seen(lthip_ingest* g, const uint32_t* d_first_index, uint64_t unique_chunks)
{
    if (!g)
        return EINVAL;
    g->ext_first = d_first_index;
    g->ext_unique = unique_chunks;
    return 0;
}

extern "C" int lthip_ingest_set_store(lthip_ingest* g, const lthip_store* store)
{
    if (!g)
        return EINVAL;
    if (store && lthip_store_ctx(store) != g->ctx)
        return lthip_fail(g->ctx, EINVAL, "lthip_ingest_set_store", "the store belongs to another context");
    g->store = store;
    return 0;
}

extern "C" int lthip_ingest_store_stats(const lthip_ingest* g, uint64_t* known_chunks, uint64_t* known_bytes)
{
    if (!g)
        return EINVAL;
    if (known_chunks)
        *known_chunks = g->store && g->indexed ? g->known_chunks : 0;
    if (known_bytes)
        *known_bytes = g->store && g->indexed ? g->known_bytes : 0;
    return 0;
}

// Greedy packing of the owned chunks into blocks (Longtail_CreateStoreIndex :6801-6860), serial like the reference's, continued from
// where it stopped: until the new blocks hold `raw_budget` bytes or the chunks on the host (pack_avail) run out.  A block is only
// closed when the chunk that does not fit any more has been seen (or there is none).
static void ingest_pack(lthip_ingest* g, uint64_t raw_budget)
{
    const uint32_t nm = (uint32_t)g->n_mine, avail = g->pack_avail;
    const uint32_t* lens = (const uint32_t*)g->h_mu_len.p;
    const uint8_t* brk = (const uint8_t*)g->h_brk.p;
    const uint32_t* tags = g->has_tags ? (const uint32_t*)g->h_mu_tag.p : nullptr;
    const uint64_t limit = block_limit(g->cfg.max_block_size);
    const uint32_t max_chunks = g->cfg.max_chunks_per_block;
    uint64_t added = 0;
    uint32_t i = g->pack_next;
    while (i < avail && added < raw_budget)
    {
        uint64_t size;
        const uint32_t j = next_block_end(lens, tags, i, avail, max_chunks, limit, &size);
        if (j == avail && avail < nm && j - i < max_chunks)
            break; // the next chunk may still belong to this block
        g->b_size.push_back(size);
        g->b_first.push_back(j); // (b_first[b + 1]: where block b ends)
        g->b_is_range.push_back(memchr(brk + i + 1, 1, j - i - 1) ? 0 : 1); // (no chunk behind the first breaks the byte range)
        g->b_tag.push_back(tags ? tags[i] : g->cfg.compression_type);
        added += size;
        i = j;
    }
    g->pack_next = i;
    g->pack_raw += added;
}

// The rest of the packing, then the block hashes = BLAKE3 of each block's chunk-hash array (:3753-3757) on their way to the host.
// lthip_ingest_write calls this behind the launches of its first batch (the codec runs while the host packs), lthip_ingest_finish when
// nothing was written.
static int ingest_blocks_done(lthip_ingest* g)
{
    if (g->blocks_done)
        return 0;
    lthip_ctx* ctx = g->ctx;
    hipStream_t s = ctx->stream;
    int err;
    if (g->pack_avail < g->n_mine)
    {
        LTHIP_CHECK(ctx, hipEventSynchronize(g->ev_offs));
        g->pack_avail = (uint32_t)g->n_mine;
    }
    ingest_pack(g, ~0ull);
    const size_t nb = g->b_size.size();
    g->res.blocks = nb;
    g->res.raw_bytes = g->pack_raw;
    if ((err = reserve_pinned(ctx, g->h_bhash, nb * 8)) || (err = reserve_pinned(ctx, g->h_comp, nb * 4 + 8)))
        return err;
    if (nb)
    {
        BlockHashRanges r; // (with the leaves of the hash arrays, so the hash launcher reads nothing back -- the stream holds the first
                           // codec batch by now)
        r.fill(g->b_first.data(), nb, 0);
        if ((err = lthip_stage_upload(ctx, g->d_boff.p, r.off.data(), nb * 8, s)) || (err = lthip_stage_upload(ctx, g->d_blen.p, r.len.data(), nb * 4, s)))
            return err;
        if ((err = lthip_hash_ranges_by_id(ctx, g->cfg.hash_identifier, g->d_mu_hash.p, nb, (const uint64_t*)g->d_boff.p, (const uint32_t*)g->d_blen.p, r.max_len,
                                           r.leaves, (uint64_t*)g->d_bhash.p)))
            return err;
        LTHIP_CHECK(ctx, hipMemcpyAsync(g->h_bhash.p, g->d_bhash.p, nb * 8, hipMemcpyDeviceToHost, s));
    }
    LTHIP_CHECK(ctx, hipEventRecord(g->ev_index, s));
    g->blocks_done = true;
    return 0;
}

// The serialized VersionIndex into the caller's buffer: steps 2 and 3 of the builder (index_kernels.h; step 1 ran on the session's
// stream).  `ctx`: the context whose stream, staging ring and scratch it may use -- the helper thread's own, or the session's.
static int ingest_vi_work(lthip_ingest* g, lthip_ctx* ctx)
{
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx != g->ctx)
        LTHIP_CHECK(ctx, hipStreamWaitEvent(ctx->stream, g->ev_lens, 0)); // (recorded behind the first-seen pass on the session's stream)
    const uint32_t n = (uint32_t)g->n_all;
    if (const int err = lthip_vi_hashes(ctx, g->vi, g->vi_tree, g->vi_hashes, n))
        return err;
    return lthip_vi_sections(ctx, g->vi, g->vi_tree, n, g->unique_all, g->has_tags ? nullptr : &g->cfg.compression_type, g->vi_out);
}

// collects the helper (and what it queued): its error, if any
static int ingest_vi_join(lthip_ingest* g)
{
    if (g->vi_thread.joinable())
    {
        g->vi_thread.join();
        if (g->vi_ctx)
            (void)hipStreamSynchronize(g->vi_ctx->stream);
    }
    const int e = g->vi_err;
    g->vi_err = 0;
    return e;
}

// starts what lthip_ingest_index prepared (once): the helper thread, or the work itself when the thread is switched off
static int ingest_vi_start(lthip_ingest* g)
{
    if (!g->vi_pending)
        return 0;
    g->vi_pending = false;
    lthip_ctx* ctx = g->ctx;
    LTHIP_ABLATION_ENV(env_vit, "LTHIP_INGEST_VI_THREAD");
    if (env_vit.get() == 0)
        return ingest_vi_work(g, ctx);
    if (!g->vi_ctx && lthip_ctx_create(ctx->device, LTHIP_STREAM_PRIVATE, &g->vi_ctx) != 0)
        return lthip_fail(ctx, ENOMEM, "lthip_ingest", "no context for the VersionIndex helper");
    g->vi_thread = std::thread([g] { g->vi_err = ingest_vi_work(g, g->vi_ctx); });
    return 0;
}

// ---- lthip_ingest_index, step by step.  What the steps share of the call: ----
struct IndexCall
{
    const lthip_ingest_tree* t;
    const uint64_t* d_all_hashes;
    const uint32_t* d_all_lens;
    const uint64_t* d_local_offsets;
    const uint32_t* d_local_part_first;
    uint32_t n, nl, na; // chunks of all ranks, of this rank; assets
    bool all_mine;      // a single rank: the local arrays are the global ones
    uint64_t my_jobs;
};

// "reserve": the session's tables, by what their size follows
static int ingest_reserve(lthip_ingest* g, const IndexCall& c)
{
    lthip_ctx* ctx = g->ctx;
    const size_t n = c.n, nl = c.nl;
    int err = lthip_vi_reserve(ctx, g->vi, n, c.na, c.t->path_data_size);
    auto dev = [&](DBuf& b, size_t bytes) { err = err ? err : reserve_dev(ctx, b, bytes); };
    auto pin = [&](HBuf& b, size_t bytes) { err = err ? err : reserve_pinned(ctx, b, bytes); };
    dev(g->d_first, n * 4);
    dev(g->d_counts, 64);
    pin(g->h_counts, 64);
    dev(g->d_sum, 8);
    dev(g->d_gfirst, ((size_t)c.my_jobs + 1) * 4);
    // per local chunk -- and per block: the number of blocks is known when the packing ends, which is after the first codec batch was
    // queued, and a block holds at least one chunk
    for (DBuf* b : {&g->d_owned, &g->d_l2g, &g->d_mu_len, &g->d_mu_tag, &g->d_blen, &g->d_comp})
        dev(*b, nl * 4);
    for (DBuf* b : {&g->d_mu_hash, &g->d_mu_off, &g->d_bhash, &g->d_boff})
        dev(*b, nl * 8);
    dev(g->d_orank, (nl + 1) * 4);
    dev(g->d_brk, nl + 16);
    for (HBuf* b : {&g->h_mu_len, &g->h_mu_tag})
        pin(*b, nl * 4);
    for (HBuf* b : {&g->h_mu_off, &g->h_mu_hash})
        pin(*b, nl * 8);
    pin(g->h_brk, nl + 16);
    if (g->store)
    {
        dev(g->d_known, nl);
        if (!c.all_mine)
            dev(g->d_lhash, nl * 8);
    }
    return err;
}

// "first-seen": the pass over ALL chunks (:2951-2970) into d_first, the number of distinct hashes into d_counts[0] -- or the index the
// ranks computed together (lthip_ingest_set_first_seen: lthip_dedup_min_ordinal on every rank's share of the hash space), consumed here
static int ingest_first_seen(lthip_ingest* g, const IndexCall& c)
{
    lthip_ctx* ctx = g->ctx;
    if (!g->ext_first)
        return lthip_dedup_first_seen(ctx, c.n, c.d_all_hashes, (uint32_t*)g->d_first.p, (uint64_t*)g->d_counts.p);
    const uint64_t u = g->ext_unique;
    LTHIP_CHECK(ctx, hipMemcpyAsync(g->d_first.p, g->ext_first, (size_t)c.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    g->ext_first = nullptr;
    return lthip_stage_upload(ctx, g->d_counts.p, &u, 8, ctx->stream);
}

// "tables": the job layout validated and its host tables built -- 0.05-0.1 ms on the 64 GiB tree, while the first-seen pass (0.55 ms) runs
static int ingest_job_tables(lthip_ctx* ctx, const IndexCall& c, JobTables& jt)
{
    const lthip_ingest_tree* t = c.t;
    jt.starts.assign((size_t)c.na + 1, 0);
    jt.counts.assign(c.na, 0);
    for (uint64_t j = 0; j < t->job_count; ++j)
    {
        if (t->job_asset[j] >= c.na || t->job_first[j + 1] < t->job_first[j])
            return lthip_fail(ctx, EINVAL, "lthip_ingest_index", "bad job table");
        jt.counts[t->job_asset[j]] += (uint32_t)(t->job_first[j + 1] - t->job_first[j]);
    }
    for (uint32_t a = 0; a < c.na; ++a)
        jt.starts[a + 1] = jt.starts[a] + jt.counts[a];
    if (jt.starts[c.na] != c.n)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_index", "jobs do not cover the chunk arrays");
    if (c.all_mine)
        return c.nl == c.n ? 0 : lthip_fail(ctx, EINVAL, "lthip_ingest_index", "without my_jobs the local arrays are the global ones");
    jt.gfirst.resize((size_t)c.my_jobs + 1);
    uint64_t mine = 0;
    for (uint64_t m = 0; m < c.my_jobs; ++m)
    {
        const uint64_t j = t->my_jobs[m];
        if (j >= t->job_count || (m && j <= t->my_jobs[m - 1]))
            return lthip_fail(ctx, EINVAL, "lthip_ingest_index", "my_jobs must be ascending job indices");
        jt.gfirst[m] = (uint32_t)t->job_first[j];
        mine += t->job_first[j + 1] - t->job_first[j];
    }
    jt.gfirst[c.my_jobs] = 0;
    if (mine != c.nl)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_index", "own jobs do not add up to the local chunk count");
    return 0;
}

// "owned": the chunks this rank writes -- first-seen, in one of its own jobs (and not in the store), in version order: the store lookup,
// the ownership mark, the known-chunk statistics, the scan and the compaction; their number to the host (h_counts[2] + h_counts[3])
static int ingest_owned(lthip_ingest* g, const IndexCall& c)
{
    lthip_ctx* ctx = g->ctx;
    hipStream_t s = ctx->stream;
    const uint32_t nl = c.nl, blocks = (uint32_t)div_up_u64(nl, 256);
    uint64_t* d_counts = (uint64_t*)g->d_counts.p;
    volatile uint64_t* h_counts = (volatile uint64_t*)g->h_counts.p;
    const uint32_t* d_gfirst = c.all_mine ? nullptr : (const uint32_t*)g->d_gfirst.p;
    const uint32_t* d_tags = g->has_tags ? (const uint32_t*)g->vi.d_tags.p : nullptr;
    int err;
    h_counts[2] = h_counts[3] = h_counts[4] = h_counts[5] = 0;
    if (!nl)
        return 0;
    const uint8_t* d_known = nullptr; // (no store: k_ing_owned gets a null flag pointer)
    if (g->store)
    {
        const uint64_t* d_local_hashes = c.d_all_hashes; // (a single rank: the local arrays are the global ones)
        if (!c.all_mine)
        {
            LaunchTimer tm(ctx, LTHIP_K_OTHER);
            hipLaunchKernelGGL(k_ing_local_hashes, dim3(blocks), dim3(256), 0, s, c.d_local_part_first, (uint32_t)c.my_jobs, d_gfirst, nl, c.d_all_hashes,
                               (uint64_t*)g->d_lhash.p);
            LTHIP_LAUNCH_CHECK(ctx);
            d_local_hashes = (const uint64_t*)g->d_lhash.p;
        }
        if ((err = lthip_store_find(g->store, nl, d_local_hashes, (uint8_t*)g->d_known.p, nullptr)))
            return err;
        d_known = (const uint8_t*)g->d_known.p;
    }
    LaunchTimer tm(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_ing_owned, dim3(blocks), dim3(256), 0, s, (const uint32_t*)g->d_first.p, c.d_local_part_first, (uint32_t)c.my_jobs, d_gfirst, nl,
                       (uint32_t*)g->d_owned.p, (uint32_t*)g->d_l2g.p, d_known);
    if (d_known)
    {
        LTHIP_CHECK(ctx, hipMemsetAsync(d_counts + 4, 0, 16, s));
        hipLaunchKernelGGL(k_ing_known_stats, dim3(std::min(blocks, 1024u)), dim3(256), 0, s, (const uint32_t*)g->d_first.p, (const uint32_t*)g->d_l2g.p,
                           d_known, c.d_all_lens, nl, (unsigned long long*)(d_counts + 4));
        LTHIP_CHECK(ctx, hipMemcpyAsync((void*)(h_counts + 4), d_counts + 4, 16, hipMemcpyDeviceToHost, s));
    }
    if ((err = lthip_exclusive_scan_u32(ctx, (const uint32_t*)g->d_owned.p, (uint32_t*)g->d_orank.p, nl, nullptr, LTHIP_K_OTHER)))
        return err;
    hipLaunchKernelGGL(k_ing_compact, dim3(blocks), dim3(256), 0, s, (const uint32_t*)g->d_owned.p, (const uint32_t*)g->d_orank.p,
                       (const uint32_t*)g->d_l2g.p, nl, c.d_all_hashes, c.d_all_lens, c.d_local_offsets, (const uint32_t*)g->vi.d_starts.p, c.na, d_tags,
                       (uint64_t*)g->d_mu_hash.p, (uint32_t*)g->d_mu_len.p, (uint64_t*)g->d_mu_off.p, (uint32_t*)g->d_mu_tag.p);
    LTHIP_LAUNCH_CHECK(ctx);
    // number of owned chunks = orank[nl - 1] + owned[nl - 1]; the scan wrote nl entries, so read both
    LTHIP_CHECK(ctx, hipMemcpyAsync((void*)(h_counts + 2), (const uint32_t*)g->d_orank.p + (nl - 1), 4, hipMemcpyDeviceToHost, s));
    LTHIP_CHECK(ctx, hipMemcpyAsync((void*)(h_counts + 3), (const uint32_t*)g->d_owned.p + (nl - 1), 4, hipMemcpyDeviceToHost, s));
    return 0;
}

// "queued" / "counts": the one read-back of the call -- [0] distinct hashes of all ranks, [2] + [3] chunks this rank writes (u32 in the
// low halves), [4] / [5] chunks and bytes the store held -- and the wait for it
static int ingest_counts(lthip_ingest* g, const IndexCall& c, IngTrace& tr)
{
    lthip_ctx* ctx = g->ctx;
    volatile uint64_t* h_counts = (volatile uint64_t*)g->h_counts.p;
    LTHIP_CHECK(ctx, hipMemcpyAsync((void*)h_counts, g->d_counts.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    tr.mark("queued");
    LTHIP_CHECK(ctx, hipEventRecord(g->ev_counts, ctx->stream));
    LTHIP_CHECK(ctx, hipEventSynchronize(g->ev_counts));
    g->unique_all = h_counts[0];
    g->n_mine = c.nl ? (uint32_t)(h_counts[2] & 0xFFFFFFFFu) + (uint32_t)(h_counts[3] & 0xFFFFFFFFu) : 0u;
    g->known_chunks = h_counts[4];
    g->known_bytes = h_counts[5];
    return 0;
}

// "lists": the host needs the owned chunks' lengths, offsets (and tags) for the packing and the codec calls.  Of the offsets the packing
// loop reads only whether a chunk continues the range of the one before: a byte per chunk from k_ing_breaks.  The copies are 44 MB on
// the 64 GiB tree (0.8 ms of the link), and the first codec batch needs the head of the lists only: the chunks of about that batch
// are copied on the session's stream (ev_lens), the rest -- and the chunk hashes, which lthip_ingest_finish reads -- by the side
// stream next to the codec kernels (ev_offs, ev_hashes)
static int ingest_lists(lthip_ingest* g, const IndexCall& c)
{
    lthip_ctx* ctx = g->ctx;
    hipStream_t s = ctx->stream;
    const uint32_t nm = (uint32_t)g->n_mine;
    int err;
    uint32_t head = nm;
    {
        LTHIP_ABLATION_ENV(env_slices, "LTHIP_INGEST_PACK_SLICES");
        uint64_t tree_bytes = 0;
        for (uint32_t a = 0; a < c.na; ++a)
            tree_bytes += c.t->asset_sizes[a];
        if (env_slices.get() != 0 && c.n && tree_bytes > 2 * g->cfg.batch_bytes)
        {
            // chunks of one batch at the tree's mean chunk size, a quarter more, and the chunks of one more block
            const double per_byte = (double)c.n / (double)tree_bytes;
            const double want = 1.25 * per_byte * (double)g->cfg.batch_bytes + 2.0 * g->cfg.max_chunks_per_block + 4096.0;
            if (want < (double)nm)
                head = (uint32_t)want;
        }
    }
    g->pack_avail = head;
    hipStream_t s2 = s;
    if (head < nm && (err = lthip_second_stream(ctx, &s2)))
        return err;
    auto d2h_lists = [&](uint32_t c0, uint32_t c1, hipStream_t st) -> int {
        const size_t k = (size_t)c1 - c0;
        if (!k)
            return 0;
        LTHIP_CHECK(ctx, hipMemcpyAsync((uint32_t*)g->h_mu_len.p + c0, (const uint32_t*)g->d_mu_len.p + c0, k * 4, hipMemcpyDeviceToHost, st));
        LTHIP_CHECK(ctx, hipMemcpyAsync((uint8_t*)g->h_brk.p + c0, (const uint8_t*)g->d_brk.p + c0, k, hipMemcpyDeviceToHost, st));
        if (g->has_tags)
            LTHIP_CHECK(ctx, hipMemcpyAsync((uint32_t*)g->h_mu_tag.p + c0, (const uint32_t*)g->d_mu_tag.p + c0, k * 4, hipMemcpyDeviceToHost, st));
        LTHIP_CHECK(ctx, hipMemcpyAsync((uint64_t*)g->h_mu_off.p + c0, (const uint64_t*)g->d_mu_off.p + c0, k * 8, hipMemcpyDeviceToHost, st));
        return 0;
    };
    if (nm)
    {
        hipLaunchKernelGGL(k_ing_breaks, dim3((uint32_t)div_up_u64(nm, 256)), dim3(256), 0, s, (const uint64_t*)g->d_mu_off.p,
                           (const uint32_t*)g->d_mu_len.p, nm, (uint8_t*)g->d_brk.p);
        LTHIP_LAUNCH_CHECK(ctx);
        if ((err = d2h_lists(0, head, s)))
            return err;
    }
    LTHIP_CHECK(ctx, hipEventRecord(g->ev_lens, s));
    if (s2 != s)
        LTHIP_CHECK(ctx, hipStreamWaitEvent(s2, g->ev_lens, 0));
    if ((err = d2h_lists(head, nm, s2)))
        return err;
    LTHIP_CHECK(ctx, hipEventRecord(g->ev_offs, s2));
    if (nm)
        LTHIP_CHECK(ctx, hipMemcpyAsync(g->h_mu_hash.p, g->d_mu_hash.p, (size_t)nm * 8, hipMemcpyDeviceToHost, s2)); // StoreIndex, read in finish
    LTHIP_CHECK(ctx, hipEventRecord(g->ev_hashes, s2));
    return 0;
}

// "pack": greedy packing of the owned chunks (Longtail_CreateStoreIndex :6801-6860), here the blocks of the first codec batch -- once
// the head of the lists is on the host
static int ingest_pack_first(lthip_ingest* g)
{
    LTHIP_CHECK(g->ctx, hipEventSynchronize(g->ev_lens));
    g->b_first.clear();
    g->b_first.push_back(0);
    g->b_size.clear();
    g->b_is_range.clear();
    g->b_tag.clear();
    g->pack_next = 0;
    g->pack_raw = 0;
    g->blocks_done = false;
    g->written = false;
    ingest_pack(g, g->cfg.batch_bytes + 2ull * g->cfg.max_block_size);
    return 0;
}

// "helper": the VersionIndex sections are 1.2-2.4 ms of host work on the 64 GiB tree (the tables of 65 536 assets, the tag column of
// 2.1 M chunks) plus copies and two small hash launches, none of which the rest of the session waits for: a helper thread with a
// context of its own does them (LTHIP_INGEST_VI_THREAD=0: the calling thread, on the session's context), started by ingest_vi_start once
// the first codec batch is queued -- a thread's start is 0.1 ms -- and collected by lthip_ingest_finish.  Here: what it will read, the
// caller's tree as a deep copy.
static int ingest_vi_prepare(lthip_ingest* g, const IndexCall& c, ViTree view, JobTables& jt, void* h_version_index, size_t capacity)
{
    g->vi_size = lthip_version_index_size(c.na, g->unique_all, c.n, view.path_data_size);
    if (capacity < g->vi_size)
        return lthip_fail(g->ctx, ENOMEM, "lthip_ingest_index", "version index buffer too small");
    g->vi_asset_sizes.assign(view.asset_sizes, view.asset_sizes + c.na);
    g->vi_path_offsets.assign(view.path_offsets, view.path_offsets + c.na);
    g->vi_permissions.assign(view.permissions, view.permissions + c.na);
    g->vi_path_data.assign(view.path_data, view.path_data + view.path_data_size);
    g->vi_jobs.starts.swap(jt.starts);
    g->vi_jobs.counts.swap(jt.counts);
    view.asset_sizes = g->vi_asset_sizes.data();
    view.path_offsets = g->vi_path_offsets.data();
    view.permissions = g->vi_permissions.data();
    view.path_data = g->vi_path_data.data();
    view.starts = g->vi_jobs.starts.data();
    view.counts = g->vi_jobs.counts.data();
    g->vi_tree = view;
    g->vi_hashes = c.d_all_hashes;
    g->vi_out = h_version_index;
    g->vi_pending = true; // (ingest_vi_start: behind the first codec batch's launches, or in lthip_ingest_finish)
    return 0;
}

// The order of the steps is the performance design.  It holds to this:
//   * the job tables are built after the first-seen pass is queued and before anything waits: the host works while the device does;
//   * the host waits exactly three times: on entry for an index that was never finished (ingest_vi_join, ev_hashes), for the counts
//     (ev_counts), and for the head of the lists before the first packing slice (ev_lens);
//   * the VersionIndex helper is only prepared here: lthip_ingest_write starts it behind its first codec batch, or lthip_ingest_finish;
//   * what a refused call leaves untouched stays untouched: the argument and tag checks run before any state is changed, the
//     VersionIndex builder's refusals before any of its work is queued (they need the job tables);
//   * LTHIP_INGEST_TRACE prints the host time of each step under the name its function carries.
extern "C" int lthip_ingest_index(lthip_ingest* g, const lthip_ingest_tree* t, const uint64_t* d_all_hashes, const uint32_t* d_all_lens,
                                  uint64_t all_chunks, const uint64_t* d_local_offsets, const uint32_t* d_local_part_first,
                                  uint64_t local_chunks, void* h_version_index, size_t version_index_capacity)
{
    if (!g || !t || (all_chunks && (!d_all_hashes || !d_all_lens)) || (local_chunks && (!d_local_offsets || !d_local_part_first)) ||
        (t->job_count && (!t->job_asset || !t->job_first)) ||
        (t->asset_count && (!t->asset_sizes || !t->path_start_offsets || !t->permissions || !t->path_data)))
        return EINVAL;
    lthip_ctx* ctx = g->ctx;
    if (all_chunks > 0x7FFFFFF0ull || local_chunks > all_chunks)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_index", "chunk counts out of range");
    if (t->job_count && t->job_first[t->job_count] != all_chunks)
        return lthip_fail(ctx, EINVAL, "lthip_ingest_index", "job_first[job_count] must be the number of chunks");
    if (t->asset_tags) // (before any work is queued: the session stays as it is)
        for (uint32_t a = 0; a < t->asset_count; ++a)
            if (const int refused = tag_refusal(g->cfg.codec, t->asset_tags[a]))
                return lthip_fail(ctx, refused, "lthip_ingest_index", tag_refusal_text(refused));
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    g->vi_pending = false;
    (void)ingest_vi_join(g); // (an index that was never finished: its helper reads what this call is about to replace ...
    (void)hipEventSynchronize(g->ev_hashes); // ... and so does the side stream)
    IngTrace tr("lthip_ingest_index");
    const bool all_mine = t->my_jobs == nullptr;
    const IndexCall c = {t, d_all_hashes, d_all_lens, d_local_offsets, d_local_part_first, (uint32_t)all_chunks, (uint32_t)local_chunks,
                         t->asset_count, all_mine, all_mine ? t->job_count : t->my_job_count};
    g->indexed = g->written = false;
    g->n_all = c.n;
    g->n_local = c.nl;
    g->has_tags = t->asset_tags != nullptr;
    g->vi_size = 0;
    memset(&g->res, 0, sizeof g->res);
    tr.mark("checks");

    int err;
    JobTables jt;
    if ((err = ingest_reserve(g, c)))
        return err;
    tr.mark("reserve");
    if ((err = ingest_first_seen(g, c)))
        return err;
    tr.mark("first-seen");
    if ((err = ingest_job_tables(ctx, c, jt)))
        return err;
    const ViTree view = {c.na, t->asset_sizes, t->path_start_offsets, t->permissions, t->path_data, t->path_data_size, jt.counts.data(), jt.starts.data(),
                         g->cfg.hash_identifier, g->cfg.target_chunk_size};
    if (h_version_index && (err = lthip_vi_refusals(ctx, view, "lthip_ingest_index")))
        return err;
    tr.mark("tables");
    // the unique lists (the builder's step 1) and the owned chunks, on the session's stream behind the first-seen pass
    if ((!all_mine && (err = lthip_stage_upload(ctx, g->d_gfirst.p, jt.gfirst.data(), jt.gfirst.size() * 4, ctx->stream))) ||
        (err = vi_unique_lists(ctx, g->vi, (const uint32_t*)g->d_first.p, c.n, d_all_hashes, d_all_lens, jt.starts.data(), t->asset_tags, c.na)) ||
        (err = ingest_owned(g, c)) || (err = ingest_counts(g, c, tr)))
        return err;
    tr.mark("counts");
    if ((err = ingest_lists(g, c)))
        return err;
    tr.mark("lists");
    if ((err = ingest_pack_first(g)))
        return err;
    tr.mark("pack");
    if (h_version_index && (err = ingest_vi_prepare(g, c, view, jt, h_version_index, version_index_capacity)))
        return err;
    tr.mark("helper");

    g->res.chunks_all = c.n;
    g->res.unique_all = g->unique_all;
    g->res.chunks_local = c.nl;
    g->res.unique_local = g->n_mine;
    g->res.version_index_size = g->vi_size; // (blocks and raw_bytes: ingest_blocks_done)
    g->indexed = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// phase 3: WriteContent into a bounded device arena (null sink)
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int lthip_ingest_write(lthip_ingest* g, const void* d_data, void* d_arena, uint64_t arena_bytes)
{
    if (!g || !g->indexed || (g->n_mine && (!d_data || !d_arena)))
        return EINVAL;
    IngTrace tr("lthip_ingest_write");
    lthip_ctx* ctx = g->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t* lens = (const uint32_t*)g->h_mu_len.p;
    const uint64_t* offs = (const uint64_t*)g->h_mu_off.p;
    int err;
    uint64_t gathered_blocks = 0, gathered_bytes = 0;
    BlockBatch& bt = g->batch;
    bt.clear();
    g->img.set(0, bt);
    // more blocks, when the batch being put together has taken all there are and chunks are left
    auto more_blocks = [&](size_t have) -> int {
        while (g->b_size.size() == have && g->pack_next < g->n_mine)
        {
            if (g->pack_next + 2ull * g->cfg.max_chunks_per_block >= g->pack_avail && g->pack_avail < g->n_mine)
            {
                LTHIP_CHECK(ctx, hipEventSynchronize(g->ev_offs));
                g->pack_avail = (uint32_t)g->n_mine;
            }
            ingest_pack(g, 1ull << 30);
        }
        return 0;
    };
    for (size_t b0 = 0;;)
    {
        if ((err = more_blocks(b0)))
            return err;
        if (b0 == g->b_size.size())
            break;
        // ---- one batch: as many blocks as the arena and the codec's batch size hold (always at least one).  A block that is one byte
        // range of the data is compressed where it lies (place 0), every other one is assembled in d_gather first (place 1;
        // WriteContentBlockJob, :4640-4721), a range per chunk; a raw block is copied from where its chunks lie ----
        size_t b1 = b0;
        uint64_t bytes = 0, pos = 0;
        bt.clear();
        g->gather.clear();
        while ((err = more_blocks(b1)) == 0 && b1 < g->b_size.size())
        {
            const uint32_t nchunks = (uint32_t)(g->b_first[b1 + 1] - g->b_first[b1]);
            const BlockCodec bc = block_codec(g->cfg, g->b_tag[b1]);
            const uint64_t need = BlockBatch::slot(bc.codec, nchunks, g->b_size[b1]);
            if (b1 > b0 && (bt.arena + need > arena_bytes || bytes + g->b_size[b1] > g->cfg.batch_bytes))
                break;
            if (bt.arena + need > arena_bytes)
                return lthip_fail(ctx, ENOMEM, "lthip_ingest_write", "the arena does not hold a single stored block");
            const uint32_t place = bc.codec == LTHIP_CODEC_NONE ? PLACE_RAW : g->b_is_range[b1] ? 0u : 1u;
            uint64_t off = place == 0 ? offs[g->b_first[b1]] : 0;
            if (place == 1)
            {
                off = pos = (pos + 15u) & ~(uint64_t)15u;
                for (uint64_t c = g->b_first[b1]; c < g->b_first[b1 + 1]; ++c)
                {
                    g->gather.add(offs[c], lens[c], pos, 0);
                    pos += lens[c];
                }
                ++gathered_blocks;
                gathered_bytes += g->b_size[b1];
            }
            bt.add(nchunks, g->b_size[b1], g->b_tag[b1], bc, place, off);
            bytes += g->b_size[b1];
            ++b1;
        }
        if (err)
            return err;
        tr.mark("batch");
        if (pos && ((err = reserve_dev(ctx, g->d_gather, pos + 256)) || (err = lthip_gather_upload(ctx, g->wbufs, d_data, g->gather, g->d_gather.p))))
            return err;
        const BlockBatchDev dev = {{d_data, g->d_gather.p}, 2, (const uint64_t*)g->d_mu_hash.p, (const uint32_t*)g->d_mu_len.p, (uint32_t)g->b_first[b0],
                                   (const uint64_t*)g->d_mu_off.p, d_data, (const uint64_t*)g->d_bhash.p + b0, (uint32_t*)g->d_comp.p + b0, d_arena};
        if ((err = lthip_block_payloads(ctx, g->wbufs, bt, dev)))
            return err;
        tr.mark("codec");
        // ---- (first batch: the codec has work now; the rest of the packing and all block hashes) ----
        if ((err = ingest_vi_start(g)) || (err = ingest_blocks_done(g)))
            return err;
        tr.mark("blocks");
        // (a tree without asset tags: every block carries cfg.compression_type, and no tags are uploaded)
        if ((err = lthip_block_headers_upload(ctx, g->wbufs, bt, g->has_tags)) || (err = lthip_block_headers(ctx, g->wbufs, bt, dev, g->cfg, g->has_tags)))
            return err;
        g->img.set(b0, bt);
        b0 = b1;
    }
    if ((err = ingest_vi_start(g)) || (err = ingest_blocks_done(g))) // (nothing to write)
        return err;
    const size_t nb = g->b_size.size();
    // compressed sizes of all blocks: total on the device, list to the host for the caller's statistics
    LTHIP_CHECK(ctx, hipMemsetAsync(g->d_sum.p, 0, 8, s));
    if (nb)
    {
        hipLaunchKernelGGL(k_ing_sum_u32, dim3(64), dim3(256), 0, s, (const uint32_t*)g->d_comp.p, (uint32_t)nb, (unsigned long long*)g->d_sum.p);
        LTHIP_LAUNCH_CHECK(ctx);
        LTHIP_CHECK(ctx, hipMemcpyAsync((uint8_t*)g->h_comp.p + 8, g->d_comp.p, nb * 4, hipMemcpyDeviceToHost, s));
    }
    LTHIP_CHECK(ctx, hipMemcpyAsync(g->h_comp.p, g->d_sum.p, 8, hipMemcpyDeviceToHost, s));
    g->res.gathered_blocks = gathered_blocks;
    g->res.gathered_bytes = gathered_bytes;
    g->written = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// the serialized StoreIndex of what this rank wrote (Longtail_CreateStoreIndexFromBlocks :9060-9125, layout :8913-8931),
// laid out by the host while the codec is still running, then the one synchronisation of the session
// ---------------------------------------------------------------------------------------------------------------------
extern "C" int lthip_ingest_finish(lthip_ingest* g, void* h_store_index, size_t store_index_capacity, lthip_ingest_result* out)
{
    if (!g || !g->indexed)
        return EINVAL;
    lthip_ctx* ctx = g->ctx;
    // (checked before any work: a call that is going to be refused changes nothing)
    if (!result_struct_ok(out))
        return lthip_fail(ctx, EINVAL, "lthip_ingest_finish", RESULT_STRUCT_TEXT);
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    {
        int err = ingest_blocks_done(g); // (an index without lthip_ingest_write)
        if (!err)
            err = ingest_vi_start(g);
        if (err)
            return err;
    }
    const size_t nb = g->b_size.size(), m = (size_t)g->n_mine;
    const size_t size = store_index_size(nb, m);
    g->res.store_index_size = size;
    int rc = 0;
    if (h_store_index)
    {
        if (store_index_capacity < size)
            rc = ENOMEM;
        else
        {
            LTHIP_CHECK(ctx, hipEventSynchronize(g->ev_index));  // block hashes ...
            LTHIP_CHECK(ctx, hipEventSynchronize(g->ev_hashes)); // ... and the owned chunks' hashes are on the host
            write_store_index(h_store_index, g->cfg.hash_identifier, nb, m, g->h_bhash.p, g->h_mu_hash.p, g->b_first.data(), g->b_tag.data(), g->h_mu_len.p);
        }
    }
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    LTHIP_CHECK(ctx, hipEventSynchronize(g->ev_hashes)); // (the side stream's copies)
    {
        const int vi_err = ingest_vi_join(g); // the VersionIndex is in the caller's buffer (or could not be made)
        if (vi_err)
            return lthip_fail(ctx, vi_err, "lthip_ingest_finish: VersionIndex", g->vi_ctx ? g->vi_ctx->err : "");
    }
    g->res.compressed_bytes = g->written ? *(const uint64_t*)g->h_comp.p : 0;
    if (g->written)
        g->img.complete(lthip_ingest_compressed_sizes(g));
    deliver_result(out, &g->res);
    return rc;
}

extern "C" int lthip_ingest_images(const lthip_ingest* g, uint64_t* out_first_block, uint64_t* out_count, const uint64_t** out_offsets,
                                   const uint32_t** out_sizes)
{
    if (!g || !g->written)
        return EINVAL;
    g->img.get(out_first_block, out_count, out_offsets, out_sizes);
    return 0;
}

extern "C" const uint32_t* lthip_ingest_compressed_sizes(const lthip_ingest* g) { return g && g->written ? (const uint32_t*)((const uint8_t*)g->h_comp.p + 8) : nullptr; }
