// k_dedup.hip -- first-seen dedup of chunk hashes on gfx950.
//
// Reference behaviour: the serial pass of Longtail_CreateVersionIndex (src/longtail.c:2951-2970):
// LookupTable_PutUnique over all chunk hashes in (asset, part, chunk) order; a chunk is "unique" the first time
// its hash appears and every later occurrence maps to that first index.  On the GPU the same mapping is the
// minimum index per key in an open-addressing table (atomicCAS on the key, atomicMin on the index), which is
// order independent, so 8 ranks that all-gather their hash arrays (RCCL) derive identical results.
#include "lthip_internal.h"

#include <algorithm>

namespace
{

constexpr uint64_t EMPTY_KEY = 0xFFFFFFFFFFFFFFFFull;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 33)) * 0xff51afd7ed558ccdull;
    z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53ull;
    return z ^ (z >> 33);
}

__global__ void k_dedup_clear(uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, uint64_t slots, uint32_t* special,
                              unsigned long long* unique)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x)
    {
        keys[i] = EMPTY_KEY;
        idx[i] = 0xFFFFFFFFu;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
    {
        *special = 0xFFFFFFFFu;
        *unique = 0ull;
    }
}

// `ordinals` (may be null): the value kept per hash is the MINIMUM of ordinals[i] instead of the minimum position i -- the
// hash-range-sharded first-seen table of the multi-GPU path, where a rank holds an arbitrary subset of the chunks and each comes
// with its global position (lthip_dedup_min_ordinal)
__global__ void k_dedup_insert(const uint64_t* __restrict__ hashes, uint64_t n, uint64_t* __restrict__ keys,
                               uint32_t* __restrict__ idx, uint64_t mask, uint32_t* special, unsigned long long* distinct,
                               const uint32_t* __restrict__ ordinals)
{
    const uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool claimed = false; // this insert claimed a slot: one more distinct hash
    if (pos < n)
    {
        const uint64_t h = hashes[pos];
        const uint32_t i = ordinals ? ordinals[pos] : (uint32_t)pos;
        if (h == EMPTY_KEY)
            claimed = atomicMin(special, i) == 0xFFFFFFFFu;
        else
        {
            uint64_t slot = mix64(h) & mask;
            for (;;)
            {
                const unsigned long long prev =
                    atomicCAS(reinterpret_cast<unsigned long long*>(&keys[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)h);
                if (prev == EMPTY_KEY || prev == h)
                {
                    atomicMin(&idx[slot], i);
                    claimed = prev == EMPTY_KEY;
                    break;
                }
                slot = (slot + 1) & mask;
            }
        }
    }
    // one add per wave (measured: not what the kernel's time is -- 0.45 ms for 2.15 M hashes either way: the CAS and the minimum are
    // 4.3 M device-scope atomics on random slots)
    const uint64_t b = __builtin_amdgcn_ballot_w64(claimed);
    if (distinct && b && (threadIdx.x & 63) == 0)
        atomicAdd(distinct, (unsigned long long)__builtin_popcountll(b));
}

__global__ void k_dedup_lookup(const uint64_t* __restrict__ hashes, uint64_t i0, uint64_t n, const uint64_t* __restrict__ keys,
                               const uint32_t* __restrict__ idx, uint64_t mask, const uint32_t* special,
                               uint32_t* __restrict__ first_index, unsigned long long* unique)
{
    const uint64_t i = i0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t mine = 0;
    if (i < i0 + n)
    {
        const uint64_t h = hashes[i];
        uint32_t f;
        if (h == EMPTY_KEY)
            f = *special;
        else
        {
            uint64_t slot = mix64(h) & mask;
            while (keys[slot] != h)
                slot = (slot + 1) & mask;
            f = idx[slot];
        }
        first_index[i - i0] = f;
        mine = f == (uint32_t)i;
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(mine != 0);
    if (unique && (threadIdx.x & 63) == 0 && b)
        atomicAdd(unique, (unsigned long long)__builtin_popcountll(b));
}

// ---- the table that is kept between calls (lthip_seen) ----
// Same slots, same probing; what differs is that a position is `base` (everything added by earlier calls) + the index in this call,
// that the table is cleared once and not per call, and that it can move into a larger one (k_seen_reinsert).
__global__ void k_seen_clear(uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, uint64_t slots)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x)
    {
        keys[i] = EMPTY_KEY;
        idx[i] = 0xFFFFFFFFu;
    }
}

__global__ void k_seen_insert(const uint64_t* __restrict__ hashes, uint64_t n, uint32_t base, uint64_t* __restrict__ keys,
                              uint32_t* __restrict__ idx, uint64_t mask, uint32_t* special, unsigned long long* distinct)
{
    const uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool claimed = false;
    if (pos < n)
    {
        const uint64_t h = hashes[pos];
        const uint32_t i = base + (uint32_t)pos;
        if (h == EMPTY_KEY)
            claimed = atomicMin(special, i) == 0xFFFFFFFFu;
        else
        {
            uint64_t slot = mix64(h) & mask;
            for (;;)
            {
                const unsigned long long prev =
                    atomicCAS(reinterpret_cast<unsigned long long*>(&keys[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)h);
                if (prev == EMPTY_KEY || prev == h)
                {
                    atomicMin(&idx[slot], i);
                    claimed = prev == EMPTY_KEY;
                    break;
                }
                slot = (slot + 1) & mask;
            }
        }
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(claimed);
    if (b && (threadIdx.x & 63) == 0)
        atomicAdd(distinct, (unsigned long long)__builtin_popcountll(b));
}

__global__ void k_seen_lookup(const uint64_t* __restrict__ hashes, uint64_t n, const uint64_t* __restrict__ keys,
                              const uint32_t* __restrict__ idx, uint64_t mask, const uint32_t* special, uint32_t* __restrict__ first_index)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t h = hashes[i];
    uint32_t f;
    if (h == EMPTY_KEY)
        f = *special;
    else
    {
        uint64_t slot = mix64(h) & mask; // (the hash was inserted by the launch before this one: the probe ends at its slot)
        while (keys[slot] != h)
            slot = (slot + 1) & mask;
        f = idx[slot];
    }
    first_index[i] = f;
}

// k_seen_lookup for hashes that may be ABSENT (lthip_seen_find): the probe ends at the key or at an empty slot, and there is one -- at
// most half of the slots are taken.  The position word of a key's slot is final once the inserts queued before this launch have run.
__global__ void k_seen_find(const uint64_t* __restrict__ hashes, uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                            uint64_t mask, const uint32_t* special, uint32_t* __restrict__ position)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t h = hashes[i];
    uint32_t f = 0xFFFFFFFFu;
    if (h == EMPTY_KEY)
        f = *special; // (0xFFFFFFFF while that hash was never added)
    else
    {
        uint64_t slot = mix64(h) & mask;
        for (;;)
        {
            const uint64_t k = keys[slot];
            if (k == h)
                f = idx[slot];
            if (k == h || k == EMPTY_KEY)
                break;
            slot = (slot + 1) & mask;
        }
    }
    position[i] = f;
}

// growth: every live (key, position) pair of the old table into the new one.  The keys of a table are distinct, so a slot of the new
// table is claimed by exactly one thread, which then owns its position word.
__global__ void k_seen_reinsert(const uint64_t* __restrict__ old_keys, const uint32_t* __restrict__ old_idx, uint64_t old_slots,
                                uint64_t* __restrict__ keys, uint32_t* __restrict__ idx, uint64_t mask)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= old_slots)
        return;
    const uint64_t h = old_keys[i];
    if (h == EMPTY_KEY)
        return;
    uint64_t slot = mix64(h) & mask;
    while (atomicCAS(reinterpret_cast<unsigned long long*>(&keys[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)h) !=
           (unsigned long long)EMPTY_KEY)
        slot = (slot + 1) & mask;
    idx[slot] = old_idx[i];
}

} // namespace

// Inserts all `count` hashes, answers for [lookup_first, lookup_first + lookup_count): d_first_index[j] = global index of the
// first occurrence of hash lookup_first + j.  *d_unique_count = number of DISTINCT hashes among all `count` (counted at
// insertion, so it does not need the lookups of the other ranks' ranges).
extern "C" int lthip_dedup_first_seen_range(lthip_ctx* ctx, uint64_t count, const uint64_t* d_hashes, uint64_t lookup_first,
                                            uint64_t lookup_count, uint32_t* d_first_index, uint64_t* d_unique_count)
{
    if (!ctx || !d_unique_count || (count && !d_hashes) || (lookup_count && !d_first_index) || lookup_first + lookup_count > count)
        return EINVAL;
    if (count > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "dedup", "too many hashes");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint64_t slots = 1024;
    while (slots < count * 2)
        slots <<= 1;
    void *keys, *idx, *misc;
    int err;
    if ((err = lthip_scratch(ctx, S_TABLES, slots * 8, &keys)))
        return err;
    if ((err = lthip_scratch(ctx, S_TABLES2, slots * 4, &idx)))
        return err;
    if ((err = lthip_scratch(ctx, S_MISC, 64, &misc)))
        return err;
    uint32_t* special = (uint32_t*)misc;
    LaunchTimer t(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_dedup_clear, dim3(2048), dim3(256), 0, ctx->stream, (uint64_t*)keys, (uint32_t*)idx, slots, special,
                       (unsigned long long*)d_unique_count);
    if (count)
        hipLaunchKernelGGL(k_dedup_insert, dim3((uint32_t)div_up_u64(count, 256)), dim3(256), 0, ctx->stream, d_hashes, count,
                           (uint64_t*)keys, (uint32_t*)idx, slots - 1, special, (unsigned long long*)d_unique_count, (const uint32_t*)nullptr);
    if (lookup_count)
        hipLaunchKernelGGL(k_dedup_lookup, dim3((uint32_t)div_up_u64(lookup_count, 256)), dim3(256), 0, ctx->stream, d_hashes,
                           lookup_first, lookup_count, (const uint64_t*)keys, (const uint32_t*)idx, slots - 1, (const uint32_t*)special,
                           d_first_index, (unsigned long long*)nullptr);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int lthip_dedup_first_seen(lthip_ctx* ctx, uint64_t count, const uint64_t* d_hashes, uint32_t* d_first_index,
                                      uint64_t* d_unique_count)
{
    if (count && !d_first_index)
        return EINVAL;
    return lthip_dedup_first_seen_range(ctx, count, d_hashes, 0, count, d_first_index, d_unique_count);
}

// The sharded form: THIS rank owns an arbitrary subset of all chunks' hashes (those of its hash range), each with its global
// position; d_first_ordinal[j] = the smallest position among the items with the hash of item j -- what the owner answers to the
// rank that sent item j.  *d_unique_count = distinct hashes of the subset (summed over the owners: the tree's unique chunks).
extern "C" int lthip_dedup_min_ordinal(lthip_ctx* ctx, uint64_t count, const uint64_t* d_hashes, const uint32_t* d_ordinals,
                                       uint32_t* d_first_ordinal, uint64_t* d_unique_count)
{
    if (!ctx || !d_unique_count || (count && (!d_hashes || !d_ordinals || !d_first_ordinal)))
        return EINVAL;
    if (count > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "dedup", "too many hashes");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    uint64_t slots = 1024;
    while (slots < count * 2)
        slots <<= 1;
    void *keys, *idx, *misc;
    int err;
    if ((err = lthip_scratch(ctx, S_TABLES, slots * 8, &keys)))
        return err;
    if ((err = lthip_scratch(ctx, S_TABLES2, slots * 4, &idx)))
        return err;
    if ((err = lthip_scratch(ctx, S_MISC, 64, &misc)))
        return err;
    uint32_t* special = (uint32_t*)misc;
    LaunchTimer t(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_dedup_clear, dim3(2048), dim3(256), 0, ctx->stream, (uint64_t*)keys, (uint32_t*)idx, slots, special,
                       (unsigned long long*)d_unique_count);
    if (count)
    {
        hipLaunchKernelGGL(k_dedup_insert, dim3((uint32_t)div_up_u64(count, 256)), dim3(256), 0, ctx->stream, d_hashes, count,
                           (uint64_t*)keys, (uint32_t*)idx, slots - 1, special, (unsigned long long*)d_unique_count, d_ordinals);
        hipLaunchKernelGGL(k_dedup_lookup, dim3((uint32_t)div_up_u64(count, 256)), dim3(256), 0, ctx->stream, d_hashes, (uint64_t)0, count,
                           (const uint64_t*)keys, (const uint32_t*)idx, slots - 1, (const uint32_t*)special, d_first_ordinal,
                           (unsigned long long*)nullptr);
    }
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// lthip_seen: the first-seen table of an array that arrives in pieces (include/longtail_hip.h).  Its memory is its own; the host
// counts what was added and decides from that count when the table moves into a larger one.
// ---------------------------------------------------------------------------------------------------------------------
struct lthip_seen
{
    lthip_ctx* ctx;
    uint64_t* keys;
    uint32_t* idx;
    void* misc; // [0] u32: first position of the 0xFFFF...FFFF hash (the table's empty key), [8] u64: distinct hashes
    uint64_t slots;
    uint64_t total;
    uint64_t grown;
};

static uint64_t seen_slots_for(uint64_t hashes)
{
    uint64_t slots = 1024;
    while (slots < hashes * 2)
        slots <<= 1;
    return slots;
}

static int seen_alloc_table(lthip_ctx* ctx, uint64_t slots, uint64_t** keys, uint32_t** idx)
{
    *keys = nullptr;
    *idx = nullptr;
    hipError_t e = lthip_hip_malloc((void**)keys, slots * 8);
    if (e == hipSuccess && (e = lthip_hip_malloc((void**)idx, slots * 4)) != hipSuccess)
    {
        (void)hipFree(*keys);
        *keys = nullptr;
    }
    if (e != hipSuccess)
        return lthip_fail(ctx, e == hipErrorOutOfMemory ? ENOMEM : EIO, "lthip_seen: table", hipGetErrorString(e));
    return 0;
}

extern "C" int lthip_seen_create(lthip_ctx* ctx, uint64_t expected_hashes, lthip_seen** out)
{
    if (!ctx || !out)
        return EINVAL;
    *out = nullptr;
    if (expected_hashes > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "lthip_seen_create", "too many hashes");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    lthip_seen* t = new (std::nothrow) lthip_seen();
    if (!t)
        return ENOMEM;
    t->ctx = ctx;
    t->slots = seen_slots_for(expected_hashes);
    int err = seen_alloc_table(ctx, t->slots, &t->keys, &t->idx);
    if (!err)
    {
        const hipError_t e = lthip_hip_malloc(&t->misc, 64);
        if (e != hipSuccess)
            err = lthip_fail(ctx, e == hipErrorOutOfMemory ? ENOMEM : EIO, "lthip_seen_create", hipGetErrorString(e));
    }
    if (err)
    {
        lthip_seen_destroy(t);
        return err;
    }
    LaunchTimer tm(ctx, LTHIP_K_OTHER);
    // (k_dedup_clear: the slots, the side slot of the empty key's hash and the distinct counter)
    hipLaunchKernelGGL(k_dedup_clear, dim3((uint32_t)std::min<uint64_t>(2048, div_up_u64(t->slots, 256))), dim3(256), 0, ctx->stream, t->keys,
                       t->idx, t->slots, (uint32_t*)t->misc, (unsigned long long*)((uint8_t*)t->misc + 8));
    if (hipGetLastError() != hipSuccess)
    {
        lthip_seen_destroy(t);
        return lthip_fail(ctx, EIO, "lthip_seen_create", "kernel launch");
    }
    *out = t;
    return 0;
}

extern "C" void lthip_seen_destroy(lthip_seen* t)
{
    if (!t)
        return;
    (void)hipSetDevice(t->ctx->device);
    if (t->keys || t->idx || t->misc)
        (void)hipStreamSynchronize(t->ctx->stream);
    if (t->keys)
        (void)hipFree(t->keys);
    if (t->idx)
        (void)hipFree(t->idx);
    if (t->misc)
        (void)hipFree(t->misc);
    delete t;
}

extern "C" uint64_t lthip_seen_total(const lthip_seen* t) { return t ? t->total : 0; }
extern "C" uint64_t lthip_seen_grown(const lthip_seen* t) { return t ? t->grown : 0; }

extern "C" int lthip_seen_add(lthip_seen* t, uint64_t count, const uint64_t* d_hashes, uint32_t* d_first_index, uint64_t* d_distinct)
{
    if (!t || (count && (!d_hashes || !d_first_index)))
        return EINVAL;
    lthip_ctx* ctx = t->ctx;
    if (count > 0x7FFFFFFFull || t->total + count > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "lthip_seen_add", "more than 2^31 - 1 hashes in one table");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    uint32_t* special = (uint32_t*)t->misc;
    unsigned long long* distinct = (unsigned long long*)((uint8_t*)t->misc + 8);
    if ((t->total + count) * 2 > t->slots)
    {
        // ---- growth: two slots per hash of the new total, at least twice the slots; the pairs move, the side slot and the counter stay ----
        uint64_t slots = t->slots * 2;
        while (slots < (t->total + count) * 2)
            slots <<= 1;
        uint64_t* keys;
        uint32_t* idx;
        int err;
        if ((err = seen_alloc_table(ctx, slots, &keys, &idx)))
            return err; // (nothing queued, nothing changed)
        {
            LaunchTimer tm(ctx, LTHIP_K_OTHER);
            hipLaunchKernelGGL(k_seen_clear, dim3((uint32_t)std::min<uint64_t>(2048, div_up_u64(slots, 256))), dim3(256), 0, s, keys, idx, slots);
            hipLaunchKernelGGL(k_seen_reinsert, dim3((uint32_t)div_up_u64(t->slots, 256)), dim3(256), 0, s, (const uint64_t*)t->keys,
                               (const uint32_t*)t->idx, t->slots, keys, idx, slots - 1);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = lthip_stream_wait(ctx); // the old table is read until here
        if (e != hipSuccess)
        {
            (void)hipFree(keys);
            (void)hipFree(idx);
            return lthip_fail(ctx, EIO, "lthip_seen_add: growth", hipGetErrorString(e));
        }
        (void)hipFree(t->keys);
        (void)hipFree(t->idx);
        t->keys = keys;
        t->idx = idx;
        t->slots = slots;
        ++t->grown;
    }
    if (count)
    {
        // insert and look-up stay two launches: a look-up beside the inserts could read a position that a later insert still lowers
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        const uint32_t blocks = (uint32_t)div_up_u64(count, 256);
        hipLaunchKernelGGL(k_seen_insert, dim3(blocks), dim3(256), 0, s, d_hashes, count, (uint32_t)t->total, t->keys, t->idx, t->slots - 1,
                           special, distinct);
        hipLaunchKernelGGL(k_seen_lookup, dim3(blocks), dim3(256), 0, s, d_hashes, count, (const uint64_t*)t->keys, (const uint32_t*)t->idx,
                           t->slots - 1, (const uint32_t*)special, d_first_index);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if (d_distinct)
        LTHIP_CHECK(ctx, hipMemcpyAsync(d_distinct, distinct, 8, hipMemcpyDeviceToDevice, s));
    t->total += count;
    return 0;
}

extern "C" int lthip_seen_find(const lthip_seen* t, uint64_t count, const uint64_t* d_hashes, uint32_t* d_position)
{
    if (!t || (count && (!d_hashes || !d_position)))
        return EINVAL;
    lthip_ctx* ctx = t->ctx;
    if (count > 0x7FFFFFFFull * 256u)
        return lthip_fail(ctx, EINVAL, "lthip_seen_find", "too many hashes in one call");
    if (!count)
        return 0;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LaunchTimer tm(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_seen_find, dim3((uint32_t)div_up_u64(count, 256)), dim3(256), 0, ctx->stream, d_hashes, count, (const uint64_t*)t->keys,
                       (const uint32_t*)t->idx, t->slots - 1, (const uint32_t*)t->misc, d_position);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// lthip_store: the set of chunk hashes a store already holds (include/longtail_hip.h) -- what the ingest sessions ask "does the store
// lack this chunk?".  Same slots, same probing and the same growth as lthip_seen, but a slot is the key alone: membership needs no
// position, and a store can hold far more chunks than a version, so neither lthip_seen's uint32_t positions nor its 2^31 - 1 total
// apply here.  The 0xFFFF...FFFF hash (the empty key) lives in a side flag.
// ---------------------------------------------------------------------------------------------------------------------
namespace
{

__global__ void k_store_clear(uint64_t* __restrict__ keys, uint64_t slots)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x)
        keys[i] = EMPTY_KEY;
}

__global__ void k_store_insert(const uint64_t* __restrict__ hashes, uint64_t n, uint64_t* __restrict__ keys, uint64_t mask, uint32_t* special,
                               unsigned long long* distinct)
{
    const uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool claimed = false;
    if (pos < n)
    {
        const uint64_t h = hashes[pos];
        if (h == EMPTY_KEY)
            claimed = atomicCAS(special, 0u, 1u) == 0u;
        else
        {
            uint64_t slot = mix64(h) & mask;
            for (;;)
            {
                const unsigned long long prev =
                    atomicCAS(reinterpret_cast<unsigned long long*>(&keys[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)h);
                if (prev == EMPTY_KEY || prev == h)
                {
                    claimed = prev == EMPTY_KEY;
                    break;
                }
                slot = (slot + 1) & mask;
            }
        }
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(claimed);
    if (b && (threadIdx.x & 63) == 0)
        atomicAdd(distinct, (unsigned long long)__builtin_popcountll(b));
}

// one thread per query; the probe ends at the key or at an empty slot, and there is one: at most half of the slots are taken
__global__ void k_store_find(const uint64_t* __restrict__ hashes, uint64_t n, const uint64_t* __restrict__ keys, uint64_t mask,
                             const uint32_t* special, uint8_t* __restrict__ known, unsigned long long* known_count)
{
    const uint64_t pos = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool hit = false;
    if (pos < n)
    {
        const uint64_t h = hashes[pos];
        if (h == EMPTY_KEY)
            hit = *special != 0u;
        else
        {
            uint64_t slot = mix64(h) & mask;
            for (;;)
            {
                const uint64_t k = keys[slot];
                if (k == h || k == EMPTY_KEY)
                {
                    hit = k == h;
                    break;
                }
                slot = (slot + 1) & mask;
            }
        }
        known[pos] = hit ? 1 : 0;
    }
    const uint64_t b = __builtin_amdgcn_ballot_w64(hit);
    if (known_count && b && (threadIdx.x & 63) == 0)
        atomicAdd(known_count, (unsigned long long)__builtin_popcountll(b));
}

// growth: every live key of the old table into the new one (the keys of a table are distinct: a slot is claimed by exactly one thread)
__global__ void k_store_reinsert(const uint64_t* __restrict__ old_keys, uint64_t old_slots, uint64_t* __restrict__ keys, uint64_t mask)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= old_slots)
        return;
    const uint64_t h = old_keys[i];
    if (h == EMPTY_KEY)
        return;
    uint64_t slot = mix64(h) & mask;
    while (atomicCAS(reinterpret_cast<unsigned long long*>(&keys[slot]), (unsigned long long)EMPTY_KEY, (unsigned long long)h) !=
           (unsigned long long)EMPTY_KEY)
        slot = (slot + 1) & mask;
}

constexpr uint64_t STORE_LAUNCH_ITEMS = 1ull << 30; // items of one launch (a thread each): a larger call is several launches

} // namespace

struct lthip_store
{
    lthip_ctx* ctx;
    uint64_t* keys;
    void* misc;      // [0] u32: the store holds the 0xFFFF...FFFF hash (the table's empty key), [8] u64: distinct hashes
    uint64_t* d_tmp; // lthip_store_add_index: the index's chunk hashes on the device
    uint64_t tmp_cap;
    uint64_t slots;
    uint64_t added;
    uint64_t grown;
};

static int store_alloc(lthip_ctx* ctx, size_t bytes, void** p, const char* what)
{
    *p = nullptr;
    const hipError_t e = lthip_hip_malloc(p, bytes);
    if (e != hipSuccess)
        return lthip_fail(ctx, e == hipErrorOutOfMemory ? ENOMEM : EIO, what, hipGetErrorString(e));
    return 0;
}

extern "C" int lthip_store_create(lthip_ctx* ctx, uint64_t expected_hashes, lthip_store** out)
{
    if (!ctx || !out)
        return EINVAL;
    *out = nullptr;
    if (expected_hashes > (1ull << 56))
        return lthip_fail(ctx, EINVAL, "lthip_store_create", "too many hashes");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    lthip_store* t = new (std::nothrow) lthip_store();
    if (!t)
        return ENOMEM;
    t->ctx = ctx;
    t->slots = seen_slots_for(expected_hashes);
    int err = store_alloc(ctx, t->slots * 8, (void**)&t->keys, "lthip_store_create");
    if (!err)
        err = store_alloc(ctx, 64, &t->misc, "lthip_store_create");
    if (!err)
    {
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_store_clear, dim3((uint32_t)std::min<uint64_t>(2048, div_up_u64(t->slots, 256))), dim3(256), 0, ctx->stream, t->keys,
                           t->slots);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemsetAsync(t->misc, 0, 64, ctx->stream);
        if (e != hipSuccess)
            err = lthip_fail(ctx, EIO, "lthip_store_create", hipGetErrorString(e));
    }
    if (err)
    {
        lthip_store_destroy(t);
        return err;
    }
    *out = t;
    return 0;
}

extern "C" void lthip_store_destroy(lthip_store* t)
{
    if (!t)
        return;
    (void)hipSetDevice(t->ctx->device);
    if (t->keys || t->misc || t->d_tmp)
        (void)hipStreamSynchronize(t->ctx->stream);
    if (t->keys)
        (void)hipFree(t->keys);
    if (t->misc)
        (void)hipFree(t->misc);
    if (t->d_tmp)
        (void)hipFree(t->d_tmp);
    delete t;
}

extern "C" uint64_t lthip_store_added(const lthip_store* t) { return t ? t->added : 0; }
extern "C" uint64_t lthip_store_grown(const lthip_store* t) { return t ? t->grown : 0; }

// room for `count` more hashes: two slots per hash of the new running total, at least twice the slots; the keys move, the side flag and
// the counter stay.  A failure leaves the table as it was.
static int store_make_room(lthip_store* t, uint64_t count)
{
    lthip_ctx* ctx = t->ctx;
    if (count > (1ull << 56) || t->added + count > (1ull << 56))
        return lthip_fail(ctx, EINVAL, "lthip_store_add", "too many hashes");
    if ((t->added + count) * 2 <= t->slots)
        return 0;
    uint64_t slots = t->slots * 2;
    while (slots < (t->added + count) * 2)
        slots <<= 1;
    uint64_t* keys;
    int err;
    if ((err = store_alloc(ctx, slots * 8, (void**)&keys, "lthip_store_add: table")))
        return err; // (nothing queued, nothing changed)
    {
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_store_clear, dim3((uint32_t)std::min<uint64_t>(2048, div_up_u64(slots, 256))), dim3(256), 0, ctx->stream, keys, slots);
        hipLaunchKernelGGL(k_store_reinsert, dim3((uint32_t)div_up_u64(t->slots, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)t->keys, t->slots,
                           keys, slots - 1);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = lthip_stream_wait(ctx); // the old table is read until here
    if (e != hipSuccess)
    {
        (void)hipFree(keys);
        return lthip_fail(ctx, EIO, "lthip_store_add: growth", hipGetErrorString(e));
    }
    (void)hipFree(t->keys);
    t->keys = keys;
    t->slots = slots;
    ++t->grown;
    return 0;
}

static int store_insert(lthip_store* t, uint64_t count, const uint64_t* d_hashes)
{
    lthip_ctx* ctx = t->ctx;
    LaunchTimer tm(ctx, LTHIP_K_OTHER);
    for (uint64_t i = 0; i < count; i += STORE_LAUNCH_ITEMS)
    {
        const uint64_t k = std::min(STORE_LAUNCH_ITEMS, count - i);
        hipLaunchKernelGGL(k_store_insert, dim3((uint32_t)div_up_u64(k, 256)), dim3(256), 0, ctx->stream, d_hashes + i, k, t->keys, t->slots - 1,
                           (uint32_t*)t->misc, (unsigned long long*)((uint8_t*)t->misc + 8));
    }
    LTHIP_LAUNCH_CHECK(ctx);
    t->added += count;
    return 0;
}

extern "C" int lthip_store_add(lthip_store* t, uint64_t count, const uint64_t* d_hashes)
{
    if (!t || (count && !d_hashes))
        return EINVAL;
    lthip_ctx* ctx = t->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    int err;
    if ((err = store_make_room(t, count)))
        return err;
    return store_insert(t, count, d_hashes);
}

extern "C" int lthip_store_add_index(lthip_store* t, const void* store_index, size_t size)
{
    if (!t || !store_index)
        return EINVAL;
    lthip_ctx* ctx = t->ctx;
    // the layout as lthip_get_existing_store_index reads it (src/longtail.c:8913-8931): [version, hash id, blocks, chunks], block hashes,
    // chunk hashes, ...
    if (size < 16)
        return lthip_fail(ctx, EBADF, "lthip_store_add_index", "store index shorter than its header");
    uint32_t head[4];
    memcpy(head, store_index, 16);
    const uint64_t nb = head[2], m = head[3];
    if (head[0] != (1u << 24)) // LONGTAIL_STORE_INDEX_VERSION_1_0_0 (src/longtail.c:19-23)
        return lthip_fail(ctx, EBADF, "lthip_store_add_index", "unsupported store index version");
    if (size < 16 + nb * 8 + m * 8 + nb * 12 + m * 4)
        return lthip_fail(ctx, EBADF, "lthip_store_add_index", "store index truncated");
    if (!m)
        return 0;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    int err;
    if (t->tmp_cap < m)
    {
        // (the buffer of the call before may still be read by its inserts: hipFree waits for them)
        uint64_t* p;
        if ((err = store_alloc(ctx, m * 8, (void**)&p, "lthip_store_add_index")))
            return err;
        if (t->d_tmp)
            (void)hipFree(t->d_tmp);
        t->d_tmp = p;
        t->tmp_cap = m;
    }
    if ((err = store_make_room(t, m)))
        return err;
    // through the staging ring in pieces, so that no staging slot grows to the size of a store's index
    const uint8_t* src = (const uint8_t*)store_index + 16 + nb * 8;
    constexpr uint64_t PIECE = 4u << 20;
    for (uint64_t o = 0; o < m * 8; o += PIECE)
        if ((err = lthip_stage_upload(ctx, (uint8_t*)t->d_tmp + o, src + o, (size_t)std::min(PIECE, m * 8 - o), ctx->stream)))
            return err;
    return store_insert(t, m, t->d_tmp);
}

extern "C" int lthip_store_find(const lthip_store* t, uint64_t count, const uint64_t* d_hashes, uint8_t* d_known, uint64_t* d_known_count)
{
    if (!t || (count && (!d_hashes || !d_known)))
        return EINVAL;
    lthip_ctx* ctx = t->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (d_known_count)
        LTHIP_CHECK(ctx, hipMemsetAsync(d_known_count, 0, 8, ctx->stream)); // (set by the call, not accumulated)
    if (!count)
        return 0;
    LaunchTimer tm(ctx, LTHIP_K_OTHER);
    for (uint64_t i = 0; i < count; i += STORE_LAUNCH_ITEMS)
    {
        const uint64_t k = std::min(STORE_LAUNCH_ITEMS, count - i);
        hipLaunchKernelGGL(k_store_find, dim3((uint32_t)div_up_u64(k, 256)), dim3(256), 0, ctx->stream, d_hashes + i, k, (const uint64_t*)t->keys,
                           t->slots - 1, (const uint32_t*)t->misc, d_known + i, (unsigned long long*)d_known_count);
    }
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int lthip_store_distinct(lthip_store* t, uint64_t* out)
{
    if (!t || !out)
        return EINVAL;
    lthip_ctx* ctx = t->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LTHIP_CHECK(ctx, hipMemcpyAsync(out, (const uint8_t*)t->misc + 8, 8, hipMemcpyDeviceToHost, ctx->stream));
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    return 0;
}

lthip_ctx* lthip_store_ctx(const lthip_store* t) { return t->ctx; }
