// k_blake2s.hip -- BLAKE2s-64 on gfx950: the 'blk2' hash type of longtail.
//
// Reference behaviour: Blake2Hash_HashBuffer / _BeginContext / _Hash / _EndContext (lib/blake2/longtail_blake2.c) =
// unkeyed BLAKE2s with outlen 8 (parameter word 0 = 0x01010008), the counter counts bytes, the last block (possibly empty,
// zero-padded) carries f0 = ~0; the digest is the first 8 output bytes as a little-endian u64 (RFC 7693 §3.2; the same
// function as Python's hashlib.blake2s(data, digest_size=8)).
//
// BLAKE2s is one serial chain of compressions per message (no tree), so two formulations:
//   lane per range   k_b2s_lanes: the 16 state + 16 message words of one range live in VGPRs, the 10 rounds are unrolled with
//                    the SIGMA schedule folded into register names, rotations are v_alignbit (as b3_g, k_blake3.hip).  Ranges
//                    start at any byte: message words are rebuilt from aligned dwords with one v_alignbit each, and the next
//                    block's loads are in flight while the current one is compressed.  Lanes take the ranges in an order sorted
//                    by length class (k_b2s_class_*, lthip_hash.hip: a device-side counting sort of ceil(len / 64) into 4 classes per octave,
//                    longest first), so the lanes of a wave run near-equal numbers of compressions.  Throughput path.  (The sort
//                    is shared with Meow, k_meow.hip, which counts 256-byte blocks: lthip_len_class_order.)
//   quad per message the four lanes of a quad hold the four columns (lane i: v[i], v[4+i], v[8+i], v[12+i]); the diagonal step
//                    is a DPP quad rotation of rows 1..3 before and after.  A compression is ~1/4 of the dependent instructions of
//                    the lane form.  Latency path: one input of up to 64 KiB (k_b2s_one), few long ranges (k_b2s_quads), the
//                    streaming pair (k_b2s_stream).
#include "lthip_internal.h"
#include "k_hash_common.h"

namespace
{

#define B2_IV0 0x6A09E667u
#define B2_IV1 0xBB67AE85u
#define B2_IV2 0x3C6EF372u
#define B2_IV3 0xA54FF53Au
#define B2_IV4 0x510E527Fu
#define B2_IV5 0x9B05688Cu
#define B2_IV6 0x1F83D9ABu
#define B2_IV7 0x5BE0CD19u
#define B2_PARAM0 0x01010008u // digest length 8, key length 0, fanout 1, depth 1

// RFC 7693 §2.7
__constant__ uint8_t B2_SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},  {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},  {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},  {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},  {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},  {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

__device__ __forceinline__ uint32_t rotr32(uint32_t x, uint32_t r) { return __builtin_amdgcn_alignbit(x, x, r); }

__device__ __forceinline__ void b2_g(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t mx, uint32_t my)
{
    a = a + b + mx;
    d = rotr32(d ^ a, 16);
    c = c + d;
    b = rotr32(b ^ c, 12);
    a = a + b + my;
    d = rotr32(d ^ a, 8);
    c = c + d;
    b = rotr32(b ^ c, 7);
}

#define B2_ROUND(m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13, m14, m15) \
    b2_g(s0, s4, s8, s12, m0, m1);                                                      \
    b2_g(s1, s5, s9, s13, m2, m3);                                                      \
    b2_g(s2, s6, s10, s14, m4, m5);                                                     \
    b2_g(s3, s7, s11, s15, m6, m7);                                                     \
    b2_g(s0, s5, s10, s15, m8, m9);                                                     \
    b2_g(s1, s6, s11, s12, m10, m11);                                                   \
    b2_g(s2, s7, s8, s13, m12, m13);                                                    \
    b2_g(s3, s4, s9, s14, m14, m15);

// h <- compress(h, m, t, f0): one lane, all sixteen words
__device__ __forceinline__ void b2_compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint32_t t_lo, uint32_t t_hi, uint32_t f0)
{
    uint32_t s0 = h[0], s1 = h[1], s2 = h[2], s3 = h[3], s4 = h[4], s5 = h[5], s6 = h[6], s7 = h[7];
    uint32_t s8 = B2_IV0, s9 = B2_IV1, s10 = B2_IV2, s11 = B2_IV3;
    uint32_t s12 = B2_IV4 ^ t_lo, s13 = B2_IV5 ^ t_hi, s14 = B2_IV6 ^ f0, s15 = B2_IV7;
    B2_ROUND(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], m[12], m[13], m[14], m[15])
    B2_ROUND(m[14], m[10], m[4], m[8], m[9], m[15], m[13], m[6], m[1], m[12], m[0], m[2], m[11], m[7], m[5], m[3])
    B2_ROUND(m[11], m[8], m[12], m[0], m[5], m[2], m[15], m[13], m[10], m[14], m[3], m[6], m[7], m[1], m[9], m[4])
    B2_ROUND(m[7], m[9], m[3], m[1], m[13], m[12], m[11], m[14], m[2], m[6], m[5], m[10], m[4], m[0], m[15], m[8])
    B2_ROUND(m[9], m[0], m[5], m[7], m[2], m[4], m[10], m[15], m[14], m[1], m[11], m[12], m[6], m[8], m[3], m[13])
    B2_ROUND(m[2], m[12], m[6], m[10], m[0], m[11], m[8], m[3], m[4], m[13], m[7], m[5], m[15], m[14], m[1], m[9])
    B2_ROUND(m[12], m[5], m[1], m[15], m[14], m[13], m[4], m[10], m[0], m[7], m[6], m[3], m[9], m[2], m[8], m[11])
    B2_ROUND(m[13], m[11], m[7], m[14], m[12], m[1], m[3], m[9], m[5], m[0], m[15], m[4], m[8], m[6], m[2], m[10])
    B2_ROUND(m[6], m[15], m[14], m[9], m[11], m[3], m[0], m[8], m[12], m[2], m[13], m[7], m[1], m[4], m[10], m[5])
    B2_ROUND(m[10], m[2], m[8], m[4], m[7], m[6], m[1], m[5], m[15], m[11], m[9], m[14], m[3], m[12], m[13], m[0])
    h[0] ^= s0 ^ s8;
    h[1] ^= s1 ^ s9;
    h[2] ^= s2 ^ s10;
    h[3] ^= s3 ^ s11;
    h[4] ^= s4 ^ s12;
    h[5] ^= s5 ^ s13;
    h[6] ^= s6 ^ s14;
    h[7] ^= s7 ^ s15;
}

// ---------------------------------------------------------------------------------------------------
// lane per range
// ---------------------------------------------------------------------------------------------------
// the raw dwords of block b: interior blocks (a byte of the range follows them) load 16 dwords + the spill-over dword when misaligned;
// the last block only the dwords that hold a byte of the range
__device__ __forceinline__ void b2_load_block(uint32_t (&w)[17], const uint32_t* q, uint32_t b, uint32_t nblocks, uint32_t mis,
                                              uint32_t len)
{
    const uint32_t* src = q + b * 16u;
    if (b + 1u < nblocks)
    {
        const u32x4_a4 v0 = *reinterpret_cast<const u32x4_a4*>(src);
        const u32x4_a4 v1 = *reinterpret_cast<const u32x4_a4*>(src + 4);
        const u32x4_a4 v2 = *reinterpret_cast<const u32x4_a4*>(src + 8);
        const u32x4_a4 v3 = *reinterpret_cast<const u32x4_a4*>(src + 12);
        w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
        w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
        w[8] = v2.x; w[9] = v2.y; w[10] = v2.z; w[11] = v2.w;
        w[12] = v3.x; w[13] = v3.y; w[14] = v3.z; w[15] = v3.w;
        w[16] = mis ? src[16] : 0u;
    }
    else
    {
        const uint32_t bl = len - b * 64u;
        const uint32_t nd = bl ? (mis + bl + 3u) >> 2 : 0u;
#pragma unroll
        for (int i = 0; i < 17; ++i)
            w[i] = (uint32_t)i < nd ? src[i] : 0u;
    }
}

__global__ __launch_bounds__(256) void k_b2s_lanes(const uint8_t* __restrict__ data, const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lens, uint64_t bound, const uint32_t* __restrict__ n_dev,
                                                   const uint32_t* __restrict__ order, const uint32_t* __restrict__ skip,
                                                   uint64_t* __restrict__ hashes)
{
    const uint32_t n = range_count(bound, n_dev);
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || (skip && g < *skip)) // (the first *skip ranges of the order are the long ones: k_b2s_quads)
        return;
    const uint32_t c = order ? order[g] : (uint32_t)g;
    const uint32_t len = lens[c];
    const uint8_t* p = data + offsets[c];
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t sh = mis * 8u;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - mis);
    const uint32_t nblocks = len ? (len + 63u) >> 6 : 1u;

    uint32_t h[8] = {B2_IV0 ^ B2_PARAM0, B2_IV1, B2_IV2, B2_IV3, B2_IV4, B2_IV5, B2_IV6, B2_IV7};
    uint32_t w[17];
    b2_load_block(w, q, 0u, nblocks, mis, len);
    for (uint32_t b = 0; b < nblocks; ++b)
    {
        const bool last = b + 1u == nblocks;
        const uint32_t bl = last ? len - b * 64u : 64u;
        uint32_t m[16];
#pragma unroll
        for (int i = 0; i < 16; ++i)
            m[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
        if (last) // zero the bytes beyond the range (the loads left whole dwords of them)
        {
#pragma unroll
            for (int i = 0; i < 16; ++i)
            {
                const int rem = (int)bl - 4 * i;
                if (rem <= 0)
                    m[i] = 0u;
                else if (rem < 4)
                    m[i] &= (1u << (8 * rem)) - 1u;
            }
        }
        if (!last)
            b2_load_block(w, q, b + 1u, nblocks, mis, len); // in flight during the compression
        const uint32_t t = last ? len : (b + 1u) * 64u; // (bytes below 4 GiB: t_hi = 0)
        b2_compress(h, m, t, 0u, last ? 0xFFFFFFFFu : 0u);
    }
    hashes[c] = (uint64_t)h[0] | ((uint64_t)h[1] << 32);
}

// ---------------------------------------------------------------------------------------------------
// quad per message
// ---------------------------------------------------------------------------------------------------
// lane i of a quad reads, per round r, message words SIGMA[r][2i], [2i+1] (column step) and SIGMA[r][8+2i], [9+2i] (diagonal step)
struct B2QuadIdx
{
    uint32_t ix[40];
};
__device__ __forceinline__ void b2_quad_idx(B2QuadIdx& q, uint32_t qi)
{
#pragma unroll
    for (int r = 0; r < 10; ++r)
    {
        q.ix[4 * r + 0] = B2_SIGMA[r][2u * qi];
        q.ix[4 * r + 1] = B2_SIGMA[r][2u * qi + 1u];
        q.ix[4 * r + 2] = B2_SIGMA[r][8u + 2u * qi];
        q.ix[4 * r + 3] = B2_SIGMA[r][9u + 2u * qi];
    }
}

// lane qi of the quad holds h[qi] (h0) and h[4 + qi] (h1); blk: the 16 message words in LDS.  All four lanes must be active.
__device__ __forceinline__ void b2_quad_compress(uint32_t& h0, uint32_t& h1, const uint32_t* blk, const B2QuadIdx& q, uint32_t qi,
                                                 uint32_t t_lo, uint32_t t_hi, uint32_t f0)
{
    uint32_t m[40];
#pragma unroll
    for (int k = 0; k < 40; ++k)
        m[k] = blk[q.ix[k]];
    const uint32_t ivc = qi == 0 ? B2_IV0 : qi == 1 ? B2_IV1 : qi == 2 ? B2_IV2 : B2_IV3;
    const uint32_t ivd = qi == 0 ? B2_IV4 ^ t_lo : qi == 1 ? B2_IV5 ^ t_hi : qi == 2 ? B2_IV6 ^ f0 : B2_IV7;
    uint32_t a = h0, b = h1, c = ivc, d = ivd;
#pragma unroll
    for (int r = 0; r < 10; ++r)
    {
        b2_g(a, b, c, d, m[4 * r + 0], m[4 * r + 1]);
        b = quad_perm<QP_ROT1>(b);
        c = quad_perm<QP_ROT2>(c);
        d = quad_perm<QP_ROT3>(d);
        b2_g(a, b, c, d, m[4 * r + 2], m[4 * r + 3]);
        b = quad_perm<QP_ROT3>(b);
        c = quad_perm<QP_ROT2>(c);
        d = quad_perm<QP_ROT1>(d);
    }
    h0 ^= a ^ c;
    h1 ^= b ^ d;
}

__device__ __forceinline__ void b2_quad_init(uint32_t& h0, uint32_t& h1, uint32_t qi)
{
    h0 = qi == 0 ? B2_IV0 ^ B2_PARAM0 : qi == 1 ? B2_IV1 : qi == 2 ? B2_IV2 : B2_IV3;
    h1 = qi == 0 ? B2_IV4 : qi == 1 ? B2_IV5 : qi == 2 ? B2_IV6 : B2_IV7;
}

// lane qi's four message words of block b of the bytes at p (any alignment), bytes at or beyond len are zero; reads only the dwords
// that hold a byte of [p, p + len)
__device__ __forceinline__ void b2_quad_raw(uint32_t (&w)[5], const uint8_t* p, uint64_t len, uint64_t b, uint32_t qi)
{
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - mis);
    const uint64_t d0 = b * 16u + qi * 4u; // first dword of the lane
    const uint64_t nd = len ? (mis + len + 3u) >> 2 : 0u;
#pragma unroll
    for (int i = 0; i < 5; ++i)
        w[i] = d0 + (uint64_t)i < nd && (i < 4 || mis) ? q[d0 + i] : 0u;
}
__device__ __forceinline__ void b2_quad_put(uint32_t* blk, const uint32_t (&w)[5], const uint8_t* p, uint64_t len, uint64_t b, uint32_t qi)
{
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u) * 8u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        uint32_t v = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
        const int64_t rem = (int64_t)len - (int64_t)(b * 64u + qi * 16u + 4u * (uint32_t)i);
        if (rem <= 0)
            v = 0u;
        else if (rem < 4)
            v &= (1u << (8 * rem)) - 1u;
        blk[qi * 4u + (uint32_t)i] = v;
    }
}

// the chain over [p, p + len) with the message staged per block through the quad's 16 LDS words; t0 = bytes hashed before p;
// final: the last block carries f0 (len 0 + final: the one empty block).  Not final: len is a non-zero multiple of 64.
__device__ void b2_quad_chain(uint32_t& h0, uint32_t& h1, const uint8_t* p, uint64_t len, uint64_t t0, bool final, uint32_t* blk,
                              const B2QuadIdx& q, uint32_t qi)
{
    const uint64_t nblocks = len ? (len + 63u) >> 6 : 1u;
    uint32_t w[5];
    b2_quad_raw(w, p, len, 0u, qi);
    for (uint64_t b = 0; b < nblocks; ++b)
    {
        const bool last = b + 1u == nblocks;
        b2_quad_put(blk, w, p, len, b, qi);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (!last)
            b2_quad_raw(w, p, len, b + 1u, qi); // in flight during the compression
        const uint64_t t = t0 + (last ? len : (b + 1u) * 64u);
        b2_quad_compress(h0, h1, blk, q, qi, (uint32_t)t, (uint32_t)(t >> 32), last && final ? 0xFFFFFFFFu : 0u);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// a quad per range (16 ranges per 64-lane workgroup): few ranges, or long ones -- a range's chain at a quarter of the lane form's latency.
// order == null: ranges 0 .. n; else the first *n_long ranges of the length-class order (the longest), grid-strided
__global__ __launch_bounds__(64) void k_b2s_quads(const uint8_t* __restrict__ data, const uint64_t* __restrict__ offsets,
                                                  const uint32_t* __restrict__ lens, uint64_t bound, const uint32_t* __restrict__ n_dev,
                                                  const uint32_t* __restrict__ order, const uint32_t* __restrict__ n_long,
                                                  uint64_t* __restrict__ hashes)
{
    __shared__ uint32_t s_blk[16 * 16];
    const uint32_t n = order ? *n_long : range_count(bound, n_dev);
    const uint32_t qi = threadIdx.x & 3u;
    B2QuadIdx q;
    b2_quad_idx(q, qi);
    for (uint64_t i = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 2); i < n; i += (uint64_t)gridDim.x * 16u) // (uniform per quad)
    {
        const uint32_t c = order ? order[i] : (uint32_t)i;
        uint32_t h0, h1;
        b2_quad_init(h0, h1, qi);
        b2_quad_chain(h0, h1, data + offsets[c], lens[c], 0u, true, s_blk + (threadIdx.x >> 2) * 16u, q, qi);
        // h[0] in lane 0, h[1] in lane 1 of the quad
        const uint32_t hi = quad_perm<QP_ROT1>(h0);
        if (qi == 0)
            hashes[c] = (uint64_t)h0 | ((uint64_t)hi << 32);
    }
}

// ONE input of at most 64 KiB, read where it lies (pinned host memory as a rule: plugin_hash.c) -- staged into LDS by the whole wave
// with coalesced 16-byte loads all in flight together (as k_blake3_one), then chained by the first quad straight from LDS.  Any start
// address: the loads are the aligned 16-byte granules that hold the input (a granule never crosses a page), and only the input's own
// bytes are kept.
__global__ __launch_bounds__(64) void k_b2s_one(const uint8_t* __restrict__ in, uint32_t len, uint64_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_in[]; // roundup(len, 64) bytes (at least one block), zero-padded
    const uint32_t lane = threadIdx.x;
    const uint32_t nblocks = len ? (len + 63u) >> 6 : 1u;
    stage_input_lds(s_in, nblocks * 16u, in, len, lane);
    if (lane >= 4u)
        return;
    B2QuadIdx q;
    b2_quad_idx(q, lane);
    uint32_t h0, h1;
    b2_quad_init(h0, h1, lane);
    for (uint32_t b = 0; b < nblocks; ++b)
    {
        const bool last = b + 1u == nblocks;
        b2_quad_compress(h0, h1, s_in + b * 16u, q, lane, last ? len : (b + 1u) * 64u, 0u, last ? 0xFFFFFFFFu : 0u);
    }
    const uint32_t hi = quad_perm<QP_ROT1>(h0);
    if (lane == 0)
        *out = (uint64_t)h0 | ((uint64_t)hi << 32);
}

// Streaming: the state in device memory is {h[0..8), bytes so far (u64)}.  A batch is a non-final run of whole blocks; the final call
// hashes the rest with f0 on its last block and writes the digest.  first: no state yet (the parameter block's h).
__global__ __launch_bounds__(64) void k_b2s_stream(const uint8_t* __restrict__ data, uint32_t len, uint32_t* __restrict__ state, int first,
                                                   int final, uint64_t* __restrict__ out)
{
    __shared__ uint32_t s_blk[16];
    const uint32_t qi = threadIdx.x;
    if (qi >= 4u)
        return;
    uint32_t h0, h1;
    uint64_t t0 = 0;
    if (first)
        b2_quad_init(h0, h1, qi);
    else
    {
        h0 = state[qi];
        h1 = state[4u + qi];
        t0 = (uint64_t)state[8] | ((uint64_t)state[9] << 32);
    }
    B2QuadIdx q;
    b2_quad_idx(q, qi);
    b2_quad_chain(h0, h1, data, len, t0, final != 0, s_blk, q, qi);
    if (final)
    {
        const uint32_t hi = quad_perm<QP_ROT1>(h0);
        if (qi == 0)
            *out = (uint64_t)h0 | ((uint64_t)hi << 32);
    }
    else
    {
        state[qi] = h0;
        state[4u + qi] = h1;
        if (qi == 0)
        {
            const uint64_t t = t0 + len;
            state[8] = (uint32_t)t;
            state[9] = (uint32_t)(t >> 32);
        }
    }
}

// the launch policy of k_hash_common.h over the four kernels
struct B2Kind
{
    static constexpr auto lanes = &k_b2s_lanes, quads = &k_b2s_quads;
    static constexpr auto one = &k_b2s_one;
    static constexpr auto stream = &k_b2s_stream;
    static constexpr int kid = LTHIP_K_BLAKE2S;
    static constexpr const char* name = "blake2s";
    static constexpr const char* name_one = "blake2s_one";
    static constexpr uint32_t unit_shift = 6u;
    // >= 1 MiB (16384 blocks): an asset's content hash over 10^5 .. 10^6 chunk hashes in a tree of many files; chunk hashing
    // (<= 2 * target bytes) never gets there
    static constexpr uint32_t long_class = 14u * 4u;
    static size_t one_lds(uint32_t len) { return (size_t)(len ? (len + 63u) >> 6 : 1u) * 64u; }
    static constexpr size_t one_lds_grant = 64u * 1024u - 1024u;
};

} // namespace

const ChainHash* lthip_chain_blake2s()
{
    static const ChainHash kind = {chain_launch_ranges<B2Kind>, chain_launch_one<B2Kind>, chain_launch_stream<B2Kind>, LTHIP_B2S_STREAM_BATCH};
    return &kind;
}
