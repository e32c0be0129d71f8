// k_blake3_leaf.h -- the BLAKE3 compression function and the hashing of ONE 1 KiB leaf in a lane's registers (device code, gfx950).
//
// Shared by k_blake3.hip (k_blake3_leaves: a thread per leaf of every range) and k_buzhash.hip (the walking scan that hashes the
// chunks it cuts, a lane per leaf).  Include inside the translation unit's anonymous namespace.
#pragma once

enum
{
    F_CHUNK_START = 1, // blake3_impl.h:14-22
    F_CHUNK_END = 2,
    F_PARENT = 4,
    F_ROOT = 8
};

#define B3_IV0 0x6A09E667u
#define B3_IV1 0xBB67AE85u
#define B3_IV2 0x3C6EF372u
#define B3_IV3 0xA54FF53Au
#define B3_IV4 0x510E527Fu
#define B3_IV5 0x9B05688Cu
#define B3_IV6 0x1F83D9ABu
#define B3_IV7 0x5BE0CD19u

__device__ __forceinline__ uint32_t b3_rotr32(uint32_t x, uint32_t r) { return __builtin_amdgcn_alignbit(x, x, r); }

__device__ __forceinline__ void b3_g(uint32_t& a, uint32_t& b, uint32_t& c, uint32_t& d, uint32_t mx, uint32_t my)
{
    a = a + b + mx;
    d = b3_rotr32(d ^ a, 16);
    c = c + d;
    b = b3_rotr32(b ^ c, 12);
    a = a + b + my;
    d = b3_rotr32(d ^ a, 8);
    c = c + d;
    b = b3_rotr32(b ^ c, 7);
}

// one round with message words named explicitly (the schedule is applied by the caller's argument order)
#define B3_ROUND(m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12, m13, m14, m15) \
    b3_g(s0, s4, s8, s12, m0, m1);                                                      \
    b3_g(s1, s5, s9, s13, m2, m3);                                                      \
    b3_g(s2, s6, s10, s14, m4, m5);                                                     \
    b3_g(s3, s7, s11, s15, m6, m7);                                                     \
    b3_g(s0, s5, s10, s15, m8, m9);                                                     \
    b3_g(s1, s6, s11, s12, m10, m11);                                                   \
    b3_g(s2, s7, s8, s13, m12, m13);                                                    \
    b3_g(s3, s4, s9, s14, m14, m15);

// cv <- first 8 output words of compress(cv, m, counter, block_len, flags)
__device__ __forceinline__ void b3_compress(uint32_t (&cv)[8], const uint32_t (&m)[16], uint32_t counter_lo,
                                            uint32_t block_len, uint32_t flags)
{
    uint32_t s0 = cv[0], s1 = cv[1], s2 = cv[2], s3 = cv[3], s4 = cv[4], s5 = cv[5], s6 = cv[6], s7 = cv[7];
    uint32_t s8 = B3_IV0, s9 = B3_IV1, s10 = B3_IV2, s11 = B3_IV3;
    uint32_t s12 = counter_lo, s13 = 0u, s14 = block_len, s15 = flags;
    // rows of MSG_SCHEDULE (blake3_impl.h:89-97): row r+1 = row r permuted by {2,6,3,10,7,0,4,13,1,11,12,5,9,14,15,8}
    B3_ROUND(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], m[12], m[13], m[14], m[15])
    B3_ROUND(m[2], m[6], m[3], m[10], m[7], m[0], m[4], m[13], m[1], m[11], m[12], m[5], m[9], m[14], m[15], m[8])
    B3_ROUND(m[3], m[4], m[10], m[12], m[13], m[2], m[7], m[14], m[6], m[5], m[9], m[0], m[11], m[15], m[8], m[1])
    B3_ROUND(m[10], m[7], m[12], m[9], m[14], m[3], m[13], m[15], m[4], m[0], m[11], m[2], m[5], m[8], m[1], m[6])
    B3_ROUND(m[12], m[13], m[9], m[11], m[15], m[10], m[14], m[8], m[7], m[2], m[5], m[3], m[0], m[1], m[6], m[4])
    B3_ROUND(m[9], m[14], m[11], m[5], m[8], m[12], m[15], m[1], m[13], m[3], m[0], m[10], m[2], m[6], m[4], m[7])
    B3_ROUND(m[11], m[15], m[5], m[0], m[1], m[9], m[8], m[6], m[14], m[10], m[2], m[12], m[3], m[4], m[7], m[13])
    cv[0] = s0 ^ s8;
    cv[1] = s1 ^ s9;
    cv[2] = s2 ^ s10;
    cv[3] = s3 ^ s11;
    cv[4] = s4 ^ s12;
    cv[5] = s5 ^ s13;
    cv[6] = s6 ^ s14;
    cv[7] = s7 ^ s15;
}

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ uint32_t leaves_of(uint32_t len) { return len ? (len + 1023u) >> 10 : 1u; }

// The message dwords of one 64-byte block as they lie in memory: 16 dwords from the 4-byte aligned address at or below the block's
// first byte, and the dword behind them, which holds the block's last 1..3 bytes when the leaf starts off a dword boundary.
__device__ __forceinline__ void b3_load_interior(uint32_t (&w)[17], const uint32_t* __restrict__ src)
{
    const u32x4_a4 v0 = *reinterpret_cast<const u32x4_a4*>(src);
    const u32x4_a4 v1 = *reinterpret_cast<const u32x4_a4*>(src + 4);
    const u32x4_a4 v2 = *reinterpret_cast<const u32x4_a4*>(src + 8);
    const u32x4_a4 v3 = *reinterpret_cast<const u32x4_a4*>(src + 12);
    w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
    w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
    w[8] = v2.x; w[9] = v2.y; w[10] = v2.z; w[11] = v2.w;
    w[12] = v3.x; w[13] = v3.y; w[14] = v3.z; w[15] = v3.w;
    // an interior block has a block of the same leaf behind it, and this is that block's first dword: it holds a byte of the leaf
    // whatever the alignment, so it is loaded without a test (v_alignbit with a shift of 0 does not look at it)
    w[16] = src[16];
}

// the leaf's last block, `nd` dwords of which hold at least one of its bytes: only those are touched
__device__ __forceinline__ void b3_load_last(uint32_t (&w)[17], const uint32_t* __restrict__ src, uint32_t nd)
{
#pragma unroll
    for (int i = 0; i < 17; ++i)
        w[i] = (uint32_t)i < nd ? src[i] : 0u;
}

// w[0 .. 15] <- the block's message words, each in the register of the dword it starts in (the dword is dead behind it): written with
// the destination tied, because left to itself the allocator puts the sixteen words into registers of their own and two sets of
// loaded dwords beside message and state then do not fit in 64
__device__ __forceinline__ void b3_interior_block(uint32_t (&cv)[8], uint32_t (&w)[17], uint32_t sh, uint32_t k, uint32_t flags)
{
#pragma unroll
    for (int i = 0; i < 16; ++i)
        asm("v_alignbit_b32 %0, %1, %0, %2" : "+v"(w[i]) : "v"(w[i + 1]), "v"(sh));
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        m[i] = w[i];
    b3_compress(cv, m, k, 64u, flags);
}

__device__ __forceinline__ void b3_last_block(uint32_t (&cv)[8], const uint32_t (&w)[17], uint32_t sh, uint32_t k, uint32_t bl, uint32_t flags)
{
    uint32_t m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        uint32_t v = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
        const int rem = (int)bl - 4 * i; // valid bytes in this word
        if (rem <= 0)
            v = 0u;
        else if (rem < 4)
            v &= (1u << (8 * rem)) - 1u;
        m[i] = v;
    }
    b3_compress(cv, m, k, bl, flags);
}

// Fixes a point of the program order: the chaining value is complete in front of it, and no load moves across it.  It emits nothing.
// (Without it the compiler sinks a whole compression below the loads that follow it, and those then need a third set of registers.)
__device__ __forceinline__ void b3_pin(uint32_t (&cv)[8])
{
    asm volatile("" : "+v"(cv[0]), "+v"(cv[1]), "+v"(cv[2]), "+v"(cv[3]), "+v"(cv[4]), "+v"(cv[5]), "+v"(cv[6]), "+v"(cv[7])::"memory");
}

// out <- the chaining value of leaf k (== the BLAKE3 chunk counter) of a range of rlen bytes, p = the leaf's first byte (any alignment):
// what a thread of k_blake3_leaves does for its leaf.  F_ROOT on the last block when the range is one leaf.
__device__ __forceinline__ void b3_leaf(uint32_t (&out)[8], const uint8_t* p, uint32_t rlen, uint32_t k)
{
    const uint32_t nleaf = leaves_of(rlen);
    const uint32_t llen = rlen - (k << 10) < 1024u ? rlen - (k << 10) : 1024u; // 0 only for the empty range
    const uint32_t root = nleaf == 1u ? (uint32_t)F_ROOT : 0u;
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t sh = mis * 8u;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - mis); // 4-byte aligned
    uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
    const uint32_t nblocks = llen ? (llen + 63u) >> 6 : 1u;
    {
#include "k_blake3_leaf_body.inc"
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        out[i] = cv[i];
}
