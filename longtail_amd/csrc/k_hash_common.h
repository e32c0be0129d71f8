// k_hash_common.h -- device helpers shared by the hash kernels that are one serial chain per message (k_blake2s.hip, k_meow.hip).
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

} // namespace
