// lthip_hash.hip -- the hash entry points of liblongtail_hip.so over inputs on the device: BLAKE3 (k_blake3.hip) and the two chain
// hashes, BLAKE2s ('blk2', k_blake2s.hip) and Meow ('meow', k_meow.hip).  The chain hashes' calls are one body each over the kind's
// descriptor (ChainHash, lthip_internal.h); what their launchers share beyond the launch policy of k_hash_common.h -- the length-class
// order of a call's ranges -- is here too, once in the code object.
#include "lthip_internal.h"
#include "k_hash_common.h"

namespace
{

// ---------------------------------------------------------------------------------------------------
// length classes: cls = 4 * floor(log2(blocks)) + the next two bits of the block count (classes 1.25x apart at most), 0 .. 127;
// a block is 1 << unit_shift bytes (BLAKE2s: 64, Meow: 256)
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t LEN_CLASSES = 128;
__device__ __forceinline__ uint32_t len_class(uint32_t len, uint32_t unit_shift)
{
    const uint32_t nb = len ? ((len - 1u) >> unit_shift) + 1u : 1u;
    const uint32_t e = 31u - (uint32_t)__builtin_clz(nb);
    const uint32_t mant = e >= 2u ? (nb >> (e - 2u)) & 3u : (nb << (2u - e)) & 3u;
    return e * 4u + mant;
}

// hist[cls] += ranges of that class (LDS histogram per workgroup, one global atomic per class)
__global__ __launch_bounds__(256) void k_b2s_class_hist(const uint32_t* __restrict__ lens, uint64_t bound, const uint32_t* __restrict__ n_dev,
                                                        uint32_t unit_shift, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t s_h[LEN_CLASSES];
    const uint32_t n = range_count(bound, n_dev);
    if (threadIdx.x < LEN_CLASSES)
        s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        atomicAdd(&s_h[len_class(lens[i], unit_shift)], 1u);
    __syncthreads();
    if (threadIdx.x < LEN_CLASSES && s_h[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], s_h[threadIdx.x]);
}

// cursor[cls] = ranges of longer classes (longest first)
__global__ __launch_bounds__(LEN_CLASSES) void k_b2s_class_scan(const uint32_t* __restrict__ hist, uint32_t* __restrict__ cursor)
{
    __shared__ uint32_t s_h[LEN_CLASSES];
    const uint32_t t = threadIdx.x;
    s_h[t] = hist[t];
    __syncthreads();
    if (t == 0)
    {
        uint32_t acc = 0;
        for (int c = (int)LEN_CLASSES - 1; c >= 0; --c)
        {
            const uint32_t v = s_h[c];
            s_h[c] = acc;
            acc += v;
        }
    }
    __syncthreads();
    cursor[t] = s_h[t];
}

// order[cursor[cls]++] = i  (the order inside a class is whatever the atomics give: every range still gets its own digest slot)
__global__ __launch_bounds__(256) void k_b2s_class_scatter(const uint32_t* __restrict__ lens, uint64_t bound, const uint32_t* __restrict__ n_dev,
                                                           uint32_t unit_shift, uint32_t* __restrict__ cursor, uint32_t* __restrict__ order)
{
    __shared__ uint32_t s_h[LEN_CLASSES], s_base[LEN_CLASSES];
    const uint32_t n = range_count(bound, n_dev);
    if (threadIdx.x < LEN_CLASSES)
        s_h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t cls = 0, rank = 0;
    if (i < n)
    {
        cls = len_class(lens[i], unit_shift);
        rank = atomicAdd(&s_h[cls], 1u);
    }
    __syncthreads();
    if (threadIdx.x < LEN_CLASSES && s_h[threadIdx.x])
        s_base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], s_h[threadIdx.x]);
    __syncthreads();
    if (i < n)
        order[s_base[cls] + rank] = (uint32_t)i;
}

} // namespace

// The length-class order of count ranges (count = min(count_bound, *d_count) when d_count != null), longest class first, in blocks of
// 1 << unit_shift bytes: *order (count_bound entries) and *n_long = the device count of ranges of class long_class and above, which
// lead the order.  S_LEN_CLASS_ORDER scratch; queued on the context's stream, nothing read back.
int lthip_len_class_order(lthip_ctx* ctx, const uint32_t* d_lens, const uint32_t* d_count, uint64_t count_bound, uint32_t unit_shift,
                          uint32_t long_class, const uint32_t** order, const uint32_t** n_long)
{
    void* sc;
    int err;
    if ((err = lthip_scratch(ctx, S_LEN_CLASS_ORDER, count_bound * 4u + 2u * LEN_CLASSES * 4u, &sc)))
        return err;
    uint32_t* hist = (uint32_t*)sc;
    uint32_t* cursor = hist + LEN_CLASSES;
    uint32_t* ord = cursor + LEN_CLASSES;
    const uint32_t grid = (uint32_t)div_up_u64(count_bound, 256);
    LTHIP_CHECK(ctx, hipMemsetAsync(hist, 0, LEN_CLASSES * 4u, ctx->stream));
    hipLaunchKernelGGL(k_b2s_class_hist, dim3(grid), dim3(256), 0, ctx->stream, d_lens, count_bound, d_count, unit_shift, hist);
    hipLaunchKernelGGL(k_b2s_class_scan, dim3(1), dim3(LEN_CLASSES), 0, ctx->stream, (const uint32_t*)hist, cursor);
    hipLaunchKernelGGL(k_b2s_class_scatter, dim3(grid), dim3(256), 0, ctx->stream, d_lens, count_bound, d_count, unit_shift, cursor, ord);
    LTHIP_LAUNCH_CHECK(ctx);
    // after the scatter cursor[c] = end of class c in the order, so cursor[long_class] = ranges of that class and above
    *order = ord;
    *n_long = cursor + long_class;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// BLAKE3
// ---------------------------------------------------------------------------------------------------
// BLAKE3-64 of runs of 64-bit values: d_out[i] = blake3(the bytes of d_values[d_first[i] .. d_first[i + 1])).  With d_values = the
// chunk hashes of lthip_chunk_hash and d_first = its part table this is every part's CONTENT hash as ChunkAssets computes it for a
// one-part asset (src/longtail.c:2518-2537): the plugin layer's batcher keeps it so that the core's later HashBuffer over the same
// digests is answered from memory (plugin_batch.c).
__global__ void k_runs_to_ranges(const uint32_t* __restrict__ first, uint32_t n, uint64_t* __restrict__ offs, uint32_t* __restrict__ lens)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
    {
        offs[i] = 8ull * first[i];
        lens[i] = 8u * (first[i + 1] - first[i]);
    }
}

extern "C" int lthip_hash_runs_u64(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                   uint64_t* d_out)
{
    return lthip_hash_runs_u64_bounded(ctx, d_values, d_first, run_count, 0, 0, d_out);
}

// runs of u64 values -> the byte ranges of the hash calls (S_TABLES scratch), shared by every hash type's runs entry points
static int runs_to_ranges(lthip_ctx* ctx, const uint32_t* d_first, uint32_t run_count, uint64_t** out_offs, uint32_t** out_lens)
{
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    void* tab;
    int err = lthip_scratch(ctx, S_TABLES, (size_t)run_count * 16, &tab);
    if (err)
        return err;
    *out_offs = (uint64_t*)tab;
    *out_lens = (uint32_t*)(*out_offs + run_count);
    hipLaunchKernelGGL(k_runs_to_ranges, dim3((run_count + 255u) / 256u), dim3(256), 0, ctx->stream, d_first, run_count, *out_offs, *out_lens);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int lthip_hash_runs_u64_bounded(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                           uint64_t total_values_bound, uint64_t run_values_bound, uint64_t* d_out)
{
    if (!ctx || !d_values || !d_first || !d_out)
        return EINVAL;
    if (run_count == 0)
        return 0;
    uint64_t* offs;
    uint32_t* lens;
    int err = runs_to_ranges(ctx, d_first, run_count, &offs, &lens);
    if (err)
        return err;
    // with the caller's bounds the launch needs nothing back from the device (no read-back, no stream synchronisation): leaves <= one per
    // KiB of values + one per run
    const uint64_t leaf_bound = total_values_bound ? total_values_bound * 8u / 1024u + run_count : 0u;
    return lthip_launch_blake3(ctx, (const uint8_t*)d_values, offs, lens, nullptr, run_count, leaf_bound, run_values_bound * 8u, d_out);
}

// Streaming BLAKE3 (k_blake3.hip): a batch of LTHIP_B3_STREAM_BATCH bytes = 1024 full leaves, the `batch_index`-th of its stream, is
// reduced to its subtree's chaining value and pushed onto the stream's stack (d_stack: LTHIP_B3_STREAM_STACK_BYTES of device memory
// owned by the caller, no initialisation needed); lthip_b3_stream_final hashes the rest (tail_len <= one batch; 0 only for an empty
// stream) and folds the stack.  The caller passes how many batches came before: the stack depth and the merges follow from that
// number alone (one entry per set bit).  The low 32 bits of the BLAKE3 chunk counter are used: streams below 4 TiB.
extern "C" int lthip_b3_stream_batch(lthip_ctx* ctx, const void* d_data, uint64_t batch_index, void* d_stack)
{
    if (!ctx || !d_data || !d_stack || batch_index >= (1ull << 22))
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t depth_in = (uint32_t)__builtin_popcountll(batch_index);
    const uint32_t merges = (uint32_t)__builtin_ctzll(batch_index + 1ull);
    return lthip_launch_blake3_stream_batch(ctx, d_data, (uint32_t)(batch_index << 10), (uint32_t*)d_stack, depth_in, merges);
}

extern "C" int lthip_b3_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, const void* d_stack,
                                     uint64_t* d_out)
{
    if (!ctx || !d_out || (tail_len && !d_tail) || tail_len > (1u << 20) || batch_count >= (1ull << 22) || (batch_count && (!tail_len || !d_stack)))
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    return lthip_launch_blake3_stream_final(ctx, d_tail, tail_len, (uint32_t)(batch_count << 10), (const uint32_t*)d_stack,
                                            (uint32_t)__builtin_popcountll(batch_count), d_out);
}

// One small input where it lies (see k_blake3_one): `in` and `out` must be readable / writable by the device -- pinned host memory
// (lthip_malloc_pinned) or device memory.  Asynchronous on the context's stream.
extern "C" int lthip_hash_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out)
{
    if (!ctx || !out || (len && !in))
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    return lthip_launch_blake3_one(ctx, in, len, out);
}

extern "C" int lthip_hash_ranges(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets,
                                 const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes)
{
    if (!ctx || (range_count && (!d_offsets || !d_lens || !d_hashes)))
        return EINVAL;
    if (range_count == 0)
        return 0;
    if (range_count > 0xFFFFFFF0ull)
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    // leaf bound unknown without reading the lengths: 0 => the launcher sizes the grid from the scanned total
    return lthip_launch_blake3(ctx, (const uint8_t*)d_data, d_offsets, d_lens, nullptr, range_count, 0, max_len, d_hashes);
}

// ... for a caller that has the lengths on the host: `leaf_total` = sum over the ranges of max(1, ceil(len / 1024)).  With ranges of
// at most 256 KiB nothing is read back and the stream is not waited for (lthip_hash_ranges stalls the caller until everything queued
// before it has run).
int lthip_hash_ranges_known(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets, const uint32_t* d_lens,
                            uint32_t max_len, uint64_t leaf_total, uint64_t* d_hashes)
{
    if (!ctx || (range_count && (!d_offsets || !d_lens || !d_hashes)) || range_count > 0xFFFFFFF0ull)
        return EINVAL;
    if (range_count == 0)
        return 0;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    return lthip_launch_blake3(ctx, (const uint8_t*)d_data, d_offsets, d_lens, nullptr, range_count, leaf_total, max_len, d_hashes);
}

// ---------------------------------------------------------------------------------------------------
// the chain hashes: one body per call over the kind's descriptor (contracts: include/longtail_hip.h)
// ---------------------------------------------------------------------------------------------------
const ChainHash* lthip_chain_hash(uint32_t hash_identifier)
{
    if (hash_identifier == LTHIP_HASH_BLAKE2)
        return lthip_chain_blake2s();
    if (hash_identifier == LTHIP_HASH_MEOW)
        return lthip_chain_meow();
    return nullptr;
}

static int chain_ranges_dev(const ChainHash* k, lthip_ctx* ctx, const void* d_data, uint64_t count_bound, const uint32_t* d_count,
                            const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes)
{
    (void)max_len; // a lane per range: the length bound does not change the launch
    if (!ctx || (count_bound && (!d_offsets || !d_lens || !d_hashes)))
        return EINVAL;
    if (count_bound == 0)
        return 0;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    return k->ranges(ctx, (const uint8_t*)d_data, d_offsets, d_lens, d_count, count_bound, d_hashes);
}

static int chain_one(const ChainHash* k, lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out)
{
    if (!ctx || !out || (len && !in))
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    return k->one(ctx, in, len, out);
}

static int chain_runs_u64_bounded(const ChainHash* k, lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                  uint64_t total_values_bound, uint64_t run_values_bound, uint64_t* d_out)
{
    (void)total_values_bound; // the bounds spare the BLAKE3 call its read-back: a chain hash never reads back
    (void)run_values_bound;
    if (!ctx || !d_values || !d_first || !d_out)
        return EINVAL;
    if (run_count == 0)
        return 0;
    uint64_t* offs;
    uint32_t* lens;
    int err = runs_to_ranges(ctx, d_first, run_count, &offs, &lens);
    if (err)
        return err;
    return k->ranges(ctx, (const uint8_t*)d_values, offs, lens, nullptr, run_count, d_out);
}

// Streaming: batch `batch_index` (k->stream_batch bytes = whole blocks of the kind, not the end of the stream) advances the state; the
// final call hashes the rest and ends the chain (BLAKE2s: the last-block flag; Meow: the total length).  Batch 0 starts the state, so
// d_state needs no initialisation.
static int chain_stream_batch(const ChainHash* k, lthip_ctx* ctx, const void* d_data, uint64_t batch_index, void* d_state)
{
    if (!ctx || !d_data || !d_state)
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    return k->stream(ctx, d_data, k->stream_batch, (uint32_t*)d_state, batch_index == 0, 0, nullptr);
}

static int chain_stream_final(const ChainHash* k, lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, void* d_state,
                              uint64_t* d_out)
{
    if (!ctx || !d_out || (tail_len && !d_tail) || tail_len > k->stream_batch || (batch_count && (!tail_len || !d_state)))
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    return k->stream(ctx, d_tail, tail_len, (uint32_t*)d_state, batch_count == 0, 1, d_out);
}

// The hash of a longtail hash type over device ranges (lthip_internal.h): the one place the index builders and the ingest session
// choose between BLAKE3 and the chain hashes.
int lthip_hash_ranges_by_id(lthip_ctx* ctx, uint32_t hash_identifier, const void* d_data, uint64_t range_count, const uint64_t* d_offsets,
                            const uint32_t* d_lens, uint32_t max_len, uint64_t leaf_total, uint64_t* d_hashes)
{
    if (const ChainHash* k = lthip_chain_hash(hash_identifier))
        return chain_ranges_dev(k, ctx, d_data, range_count, nullptr, d_offsets, d_lens, max_len, d_hashes);
    if (leaf_total)
        return lthip_hash_ranges_known(ctx, d_data, range_count, d_offsets, d_lens, max_len, leaf_total, d_hashes);
    return lthip_hash_ranges(ctx, d_data, range_count, d_offsets, d_lens, max_len, d_hashes);
}

// ---- the exported calls: BLAKE2s-64 ('blk2') ----
extern "C" int lthip_blake2s_ranges_dev(lthip_ctx* ctx, const void* d_data, uint64_t count_bound, const uint32_t* d_count,
                                        const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes)
{
    return chain_ranges_dev(lthip_chain_blake2s(), ctx, d_data, count_bound, d_count, d_offsets, d_lens, max_len, d_hashes);
}
extern "C" int lthip_blake2s_ranges(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets,
                                    const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes)
{
    return chain_ranges_dev(lthip_chain_blake2s(), ctx, d_data, range_count, nullptr, d_offsets, d_lens, max_len, d_hashes);
}
extern "C" int lthip_blake2s_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out)
{
    return chain_one(lthip_chain_blake2s(), ctx, in, len, out);
}
extern "C" int lthip_blake2s_runs_u64(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                      uint64_t* d_out)
{
    return chain_runs_u64_bounded(lthip_chain_blake2s(), ctx, d_values, d_first, run_count, 0, 0, d_out);
}
extern "C" int lthip_blake2s_runs_u64_bounded(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                              uint64_t total_values_bound, uint64_t run_values_bound, uint64_t* d_out)
{
    return chain_runs_u64_bounded(lthip_chain_blake2s(), ctx, d_values, d_first, run_count, total_values_bound, run_values_bound, d_out);
}
extern "C" int lthip_b2s_stream_batch(lthip_ctx* ctx, const void* d_data, uint64_t batch_index, void* d_state)
{
    return chain_stream_batch(lthip_chain_blake2s(), ctx, d_data, batch_index, d_state);
}
extern "C" int lthip_b2s_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, void* d_state,
                                      uint64_t* d_out)
{
    return chain_stream_final(lthip_chain_blake2s(), ctx, d_tail, tail_len, batch_count, d_state, d_out);
}

// ---- the exported calls: Meow hash v0.5, low 64 bits ('meow') ----
extern "C" int lthip_meow_ranges_dev(lthip_ctx* ctx, const void* d_data, uint64_t count_bound, const uint32_t* d_count,
                                     const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes)
{
    return chain_ranges_dev(lthip_chain_meow(), ctx, d_data, count_bound, d_count, d_offsets, d_lens, max_len, d_hashes);
}
extern "C" int lthip_meow_ranges(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets, const uint32_t* d_lens,
                                 uint32_t max_len, uint64_t* d_hashes)
{
    return chain_ranges_dev(lthip_chain_meow(), ctx, d_data, range_count, nullptr, d_offsets, d_lens, max_len, d_hashes);
}
extern "C" int lthip_meow_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out)
{
    return chain_one(lthip_chain_meow(), ctx, in, len, out);
}
extern "C" int lthip_meow_runs_u64(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count, uint64_t* d_out)
{
    return chain_runs_u64_bounded(lthip_chain_meow(), ctx, d_values, d_first, run_count, 0, 0, d_out);
}
extern "C" int lthip_meow_runs_u64_bounded(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                           uint64_t total_values_bound, uint64_t run_values_bound, uint64_t* d_out)
{
    return chain_runs_u64_bounded(lthip_chain_meow(), ctx, d_values, d_first, run_count, total_values_bound, run_values_bound, d_out);
}
extern "C" int lthip_meow_stream_batch(lthip_ctx* ctx, const void* d_data, uint64_t batch_index, void* d_state)
{
    return chain_stream_batch(lthip_chain_meow(), ctx, d_data, batch_index, d_state);
}
extern "C" int lthip_meow_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, void* d_state,
                                       uint64_t* d_out)
{
    return chain_stream_final(lthip_chain_meow(), ctx, d_tail, tail_len, batch_count, d_state, d_out);
}
