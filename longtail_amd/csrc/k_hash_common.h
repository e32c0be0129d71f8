// k_hash_common.h -- what the hashes that are one serial chain per message (k_blake2s.hip, k_meow.hip) share: device helpers of their
// kernels, and the host-side launch policy as three templates over a kind's traits.
#pragma once
#include "lthip_internal.h"

namespace
{

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// the number of ranges of a call: count_bound, or min(count_bound, *n_dev) when the count is on the device
__device__ __forceinline__ uint32_t range_count(uint64_t bound, const uint32_t* n_dev)
{
    return (uint32_t)(n_dev ? (*n_dev < bound ? *n_dev : bound) : bound);
}

template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, false);
}
constexpr int QP_ROT1 = 0x39; // lane i <- lane (i + 1) & 3
constexpr int QP_ROT2 = 0x4E; // lane i <- lane (i + 2) & 3
constexpr int QP_ROT3 = 0x93; // lane i <- lane (i + 3) & 3

// ONE input of at most 64 KiB, read where it lies (pinned host memory as a rule), staged into s_in by a whole 64-lane workgroup with
// coalesced 16-byte loads all in flight together (as k_blake3_one): s_in[0 .. zero_words) is zeroed first, then the input's bytes
// are written from its start.  Any start address: the loads are the aligned 16-byte granules that hold the input (a granule never
// crosses a page), and only the input's own bytes are kept.  Ends with a workgroup barrier.
__device__ __forceinline__ void stage_input_lds(uint32_t* s_in, uint32_t zero_words, const uint8_t* in, uint32_t len, uint32_t lane)
{
    for (uint32_t i = lane; i < zero_words; i += 64u)
        s_in[i] = 0u;
    __syncthreads();
    if (len)
    {
        const uint32_t head = (uint32_t)((uintptr_t)in & 15u);
        const uint32_t nvec = (head + len + 15u) >> 4;
        const uint4* in4 = reinterpret_cast<const uint4*>(in - head);
        uint8_t* s8 = reinterpret_cast<uint8_t*>(s_in);
        for (uint32_t v0 = 0; v0 < nvec; v0 += 64u * 8u)
        {
            uint4 qv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
            {
                const uint32_t v = v0 + (uint32_t)u * 64u + lane;
                qv[u] = v < nvec ? in4[v] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
            {
                const uint32_t v = v0 + (uint32_t)u * 64u + lane;
                if (v >= nvec)
                    continue;
                if (head == 0u && v * 16u + 16u <= len)
                    reinterpret_cast<uint4*>(s_in)[v] = qv[u];
                else
                {
                    const uint32_t w[4] = {qv[u].x, qv[u].y, qv[u].z, qv[u].w};
                    for (uint32_t k = 0; k < 16u; ++k)
                    {
                        const int64_t j = (int64_t)v * 16 + k - head; // position in the input
                        if (j >= 0 && j < (int64_t)len)
                            s8[j] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
                    }
                }
            }
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------
// host side: the launch policy of a chain hash, once.  K is the kind's traits struct, defined next to its kernels:
//   lanes, quads, one, stream   the four kernels (the same parameter lists for every kind)
//   kid                         timing id of the launches
//   name, name_one              what lthip_fail reports
//   unit_shift                  log2 of the block that the length classes count
//   long_class                  in calls of many ranges, those of this length class and above also run on quads
//   one_lds(len)                dynamic LDS bytes of the `one` kernel
//   one_lds_grant               above this many of them the kernel needs hipFuncAttributeMaxDynamicSharedMemorySize
// ---------------------------------------------------------------------------------------------------
// ranges up to this many go to the quad kernel (no sort): a call of few ranges is bound by its longest chain
constexpr uint64_t CHAIN_QUAD_RANGES = 256;
constexpr uint32_t CHAIN_LONG_GRID = 64; // workgroups of 16 quads that take the long ranges in turn

template <class K>
int chain_launch_ranges(lthip_ctx* ctx, const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_lens, const uint32_t* d_count,
                        uint64_t count_bound, uint64_t* d_hashes)
{
    if (count_bound == 0)
        return 0;
    if (count_bound > 0xFFFFFFF0ull)
        return lthip_fail(ctx, EINVAL, K::name, "too many ranges in one call");
    LaunchTimer t(ctx, K::kid);
    if (count_bound <= CHAIN_QUAD_RANGES)
    {
        hipLaunchKernelGGL(K::quads, dim3((uint32_t)div_up_u64(count_bound, 16)), dim3(64), 0, ctx->stream, d_data, d_offsets, d_lens,
                           count_bound, d_count, (const uint32_t*)nullptr, (const uint32_t*)nullptr, d_hashes);
        LTHIP_LAUNCH_CHECK(ctx);
        return 0;
    }
    const uint32_t* order;
    const uint32_t* n_long;
    int err;
    if ((err = lthip_len_class_order(ctx, d_lens, d_count, count_bound, K::unit_shift, K::long_class, &order, &n_long)))
        return err;
    hipLaunchKernelGGL(K::quads, dim3(CHAIN_LONG_GRID), dim3(64), 0, ctx->stream, d_data, d_offsets, d_lens, count_bound, d_count, order,
                       n_long, d_hashes);
    hipLaunchKernelGGL(K::lanes, dim3((uint32_t)div_up_u64(count_bound, 256)), dim3(256), 0, ctx->stream, d_data, d_offsets, d_lens,
                       count_bound, d_count, order, n_long, d_hashes);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

template <class K>
int chain_launch_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out)
{
    if (len > 65536u)
        return lthip_fail(ctx, EINVAL, K::name_one, "input above 64 KiB");
    LaunchTimer t(ctx, K::kid);
    const size_t lds = K::one_lds(len);
    if (lds > K::one_lds_grant)
    {
        static std::atomic<bool> granted[64] = {}; // per device and kind (lthip_grant_lds)
        if (int err = lthip_grant_lds(ctx, granted, {reinterpret_cast<const void*>(K::one)}, 80 * 1024))
            return err;
    }
    hipLaunchKernelGGL(K::one, dim3(1), dim3(64), lds, ctx->stream, (const uint8_t*)in, len, out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

template <class K>
int chain_launch_stream(lthip_ctx* ctx, const void* d_data, uint32_t len, uint32_t* d_state, int first, int final, uint64_t* d_out)
{
    LaunchTimer t(ctx, K::kid);
    hipLaunchKernelGGL(K::stream, dim3(1), dim3(64), 0, ctx->stream, (const uint8_t*)d_data, len, d_state, first, final, d_out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

} // namespace
