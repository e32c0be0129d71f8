// k_copy.h -- the one byte copy of the device side whose source and destination sit at any byte positions: 16-byte stores to an aligned
// destination, the source realigned from dwords with v_alignbit.  Device code only.  Used by k_gather.hip (k_gather_ranges, k_raw_copy),
// restore.hip (k_restore_scatter), lz4/lz4_stitch.inc (wg_copy) and zstd/k_zstd_common.h (wg_copy16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// four dwords at a 4-byte aligned address (and the fifth, when the source is not: it holds the last bytes of the vector) -> 16 bytes
struct RawVec
{
    u32x4_a4 a;
    uint32_t e;
};
__device__ __forceinline__ RawVec raw_load(const uint32_t* __restrict__ q, uint32_t mis)
{
    RawVec r;
    r.a = *reinterpret_cast<const u32x4_a4*>(q);
    r.e = mis ? q[4] : 0u;
    return r;
}
__device__ __forceinline__ uint4 raw_align(const RawVec& r, uint32_t sh)
{
    uint4 o;
    o.x = __builtin_amdgcn_alignbit(r.a.y, r.a.x, sh);
    o.y = __builtin_amdgcn_alignbit(r.a.z, r.a.y, sh);
    o.z = __builtin_amdgcn_alignbit(r.a.w, r.a.z, sh);
    o.w = __builtin_amdgcn_alignbit(r.e, r.a.w, sh);
    return o;
}

// THREADS threads (tid = 0 .. THREADS - 1, all of them call) copy n bytes from src to dst, both at any byte position: the head up to
// dst's 16-byte boundary and the tail by bytes, in between 16-byte stores of vectors rebuilt by raw_load / raw_align.
// THE CONTRACT that keeps every caller inside its buffers: no byte outside [dst, dst + n) is written, and no dword is read that holds no
// byte of [src, src + n).  A vector starts mis = src & 3 bytes into its first dword, so its dwords 0 .. 3 always hold bytes of it; the
// fifth is read only when mis != 0, and then it holds the vector's last mis bytes.  Head and tail read exactly their own bytes.
template <int THREADS> __device__ __forceinline__ void lthip_wg_copy(uint8_t* dst, const uint8_t* src, uint32_t n, int tid)
{
    uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
    if (head > n)
        head = n;
    if ((uint32_t)tid < head)
        dst[tid] = src[tid];
    dst += head;
    src += head;
    n -= head;
    const uint32_t nvec = n >> 4;
    const uint32_t mis = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t sh = mis * 8u;
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src - mis);
    for (uint32_t v = tid; v < nvec; v += THREADS)
        *reinterpret_cast<uint4*>(dst + (size_t)v * 16u) = raw_align(raw_load(s4 + (size_t)v * 4u, mis), sh);
    const uint32_t done = nvec << 4;
    if ((uint32_t)tid < n - done)
        dst[done + tid] = src[done + tid];
}
