// k_meow.hip -- Meow hash v0.5 on gfx950: the 'meow' hash type of longtail.
//
// Reference behaviour: MeowHash_HashBuffer / _BeginContext / _Hash / _EndContext (lib/meowhash/longtail_meowhash.c) = the streaming
// MeowBegin (default seed) / MeowAbsorb / MeowEnd of Meow hash v0.5; the digest is the low 64 bits of the 128-bit result.
//
//   state   eight 128-bit registers x0..x7, seeded with the first 256 hexadecimal digits of π.  Held as four 32-bit columns each
//           (the AES state's columns: byte i at row i % 4, column i / 4).
//   absorb  per 256-byte block, eight MIX steps, one per 32-byte lane j with the register roles (j, j+4, j+6, j+1, j+2) mod 8.  A MIX
//           of lane bytes L is  x[r1] = aesdec(x[r1], x[r2]);  x[r3] += L[15..31);  x[r2] ^= L[0..16);  x[r2] = aesdec(x[r2], x[r4]);
//           x[r5] += L[1..17);  x[r4] ^= L[16..32)   (+ = two 64-bit adds, paddq).
//   end     with Len = total bytes and R = the last Len % 256 of them: a MIX with roles 0 of the tail lane T (the last Len % 32 bytes,
//           zero-padded to 32) read at cyclic offsets 31, 0, 17, 16; one with roles 1 of the length (x[r3] += 0, x[r2] ^= 0,
//           x[r5] += Len >> 8, x[r4] ^= Len); MIXes of R's whole lanes k = 0 .. (Len >> 5) % 8 - 1 with roles k + 2; twelve
//           SHUFFLE steps; the fold x0 = ((x0 + x2) ^ (x1 + x3)) + ((x4 + x6) ^ (x5 + x7)).
//   aesdec  Intel AESDEC: InvMixColumns(InvSubBytes(InvShiftRows(a))) ^ k.  gfx950 has no AES instruction: each output column is
//           four lookups of one table TD (InvSubBytes + InvMixColumns of a row-0 byte; rows 1..3 are its byte rotations, v_alignbit)
//           and the XORs.  TD is computed at compile time from FIPS-197 (GF(2^8) inverse, affine map, coefficients 0e 0b 0d 09).
//
// TD lives in LDS, replicated: entry e of copy c at dword e * NC + c, lane l reads copy l % NC.  NC = 32 for the kernels whose 64
// lanes all look up (ds_read_b32 banks are (a/4) mod 32 per 32-lane half, so lane l always hits bank l mod 32: no conflicts, 32 KiB
// per workgroup); NC = 4 where one quad looks up (the lanes' banks differ mod 4; 4 KiB).
//
// Two formulations, as k_blake2s.hip:
//   lane per range   k_meow_lanes: one lane holds the 32 state dwords of one range; half-block loads (128 bytes) are in flight while
//                    the other half mixes.  Ranges start at any byte (lane dwords rebuilt with v_alignbit); lanes take the ranges in
//                    the length-class order of lthip_len_class_order (lthip_hash.hip) with 256-byte blocks.  Throughput path.
//   quad per message lane i of a quad holds column i of every register; InvShiftRows becomes DPP quad rotations of the input
//                    column, and paddq's carry from column 0 (2) to 1 (3) one more.  Blocks are staged through 64 LDS dwords of the
//                    quad.  Latency path: one input of up to 64 KiB (k_meow_one), few or long ranges (k_meow_quads), the streaming
//                    pair (k_meow_stream).
#include "lthip_internal.h"
#include "k_hash_common.h"

namespace
{

// ---- the AES decryption table, from FIPS-197 ----
constexpr uint32_t gf_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
    for (int i = 0; i < 8; ++i)
    {
        if (b & 1u)
            r ^= a;
        a = (a & 0x80u) ? ((a << 1) ^ 0x11Bu) : (a << 1);
        b >>= 1;
    }
    return r & 0xFFu;
}
constexpr uint32_t gf_inv(uint32_t x) // x^254 (0 -> 0)
{
    uint32_t r = 1, e = 254;
    while (e)
    {
        if (e & 1u)
            r = gf_mul(r, x);
        x = gf_mul(x, x);
        e >>= 1;
    }
    return r;
}
constexpr uint32_t aes_sbox(uint32_t x) // FIPS-197 §5.1.1: the inverse, then the affine map
{
    const uint32_t b = gf_inv(x);
    uint32_t v = b;
    for (uint32_t k = 1; k <= 4; ++k)
        v ^= ((b << k) | (b >> (8u - k))) & 0xFFu;
    return v ^ 0x63u;
}
struct MeowTable
{
    uint32_t v[256];
};
constexpr MeowTable make_td()
{
    MeowTable t{};
    uint32_t inv[256] = {};
    for (uint32_t x = 0; x < 256; ++x)
        inv[aes_sbox(x)] = x;
    for (uint32_t e = 0; e < 256; ++e) // InvMixColumns (§5.3.3) of InvSubBytes(e) in row 0, as a little-endian column
    {
        const uint32_t s = inv[e];
        t.v[e] = gf_mul(s, 0x0E) | gf_mul(s, 0x09) << 8 | gf_mul(s, 0x0D) << 16 | gf_mul(s, 0x0B) << 24;
    }
    return t;
}
constexpr MeowTable MEOW_TD_HOST = make_td();
static_assert(aes_sbox(0x00) == 0x63 && aes_sbox(0x53) == 0xED, "FIPS-197 S-box"); // §5.1.1 example
static_assert(MEOW_TD_HOST.v[0x63] == 0u, "InvSubBytes(0x63) = 0");
__constant__ MeowTable MEOW_TD = MEOW_TD_HOST;

// The default seed: π in hexadecimal, its first 256 digits, the leading 3 included, as 32 big-endian words (the seed's bytes run
// 32 43 F6 A8 88 ...; register r column c = the little-endian dword of bytes 16r + 4c ..)
__constant__ uint32_t MEOW_SEED_PI[32] = {
    0x3243F6A8, 0x885A308D, 0x313198A2, 0xE0370734, 0x4A409382, 0x2299F31D, 0x0082EFA9, 0x8EC4E6C8,
    0x9452821E, 0x638D0137, 0x7BE5466C, 0xF34E90C6, 0xCC0AC29B, 0x7C97C50D, 0xD3F84D5B, 0x5B547091,
    0x79216D5D, 0x98979FB1, 0xBD1310BA, 0x698DFB5A, 0xC2FFD72D, 0xBD01ADFB, 0x7B8E1AFE, 0xD6A267E9,
    0x6BA7C904, 0x5F12C7F9, 0x924A1994, 0x7B3916CF, 0x70801F2E, 0x2858EFC1, 0x6636920D, 0x871574E6,
};
__device__ __forceinline__ uint32_t seed_col(uint32_t r, uint32_t c) { return __builtin_bswap32(MEOW_SEED_PI[4u * r + c]); }

// TD replicated NC times into s_td (all threads of the workgroup; ends with a barrier); returns the calling lane's copy
template <uint32_t NC>
__device__ __forceinline__ const uint32_t* meow_table(uint32_t* s_td)
{
    for (uint32_t i = threadIdx.x; i < 256u * NC; i += blockDim.x)
        s_td[i] = MEOW_TD.v[i / NC];
    __syncthreads();
    return s_td + (threadIdx.x % NC);
}

template <uint32_t NC, int ROT>
__device__ __forceinline__ uint32_t td(const uint32_t* tb, uint32_t e) // TD[e] rotated left by ROT bytes
{
    const uint32_t v = tb[e * NC];
    return ROT ? __builtin_amdgcn_alignbit(v, v, 32 - 8 * ROT) : v;
}

// 16 bytes at byte O of the 32-byte lane L (8 dwords), read cyclically, as four columns
template <int O>
__device__ __forceinline__ void lane_sel(uint32_t (&o)[4], const uint32_t (&L)[8])
{
#pragma unroll
    for (int j = 0; j < 4; ++j)
        o[j] = (O & 3) ? __builtin_amdgcn_alignbyte(L[(O / 4 + j + 1) & 7], L[(O / 4 + j) & 7], O & 3) : L[(O / 4 + j) & 7];
}

// ---------------------------------------------------------------------------------------------------
// lane per range: x[r][c] = column c of register r
// ---------------------------------------------------------------------------------------------------
template <uint32_t NC>
__device__ __forceinline__ void aesdec4(uint32_t (&a)[4], const uint32_t (&k)[4], const uint32_t* tb)
{
    uint32_t o[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) // InvShiftRows: row r of column c comes from column c - r
        o[c] = td<NC, 0>(tb, a[c] & 255u) ^ td<NC, 1>(tb, (a[(c + 3) & 3] >> 8) & 255u) ^ td<NC, 2>(tb, (a[(c + 2) & 3] >> 16) & 255u) ^
               td<NC, 3>(tb, a[(c + 1) & 3] >> 24) ^ k[c];
#pragma unroll
    for (int c = 0; c < 4; ++c)
        a[c] = o[c];
}

__device__ __forceinline__ void paddq4(uint32_t (&a)[4], const uint32_t (&b)[4])
{
    const uint64_t lo = ((uint64_t)a[1] << 32 | a[0]) + ((uint64_t)b[1] << 32 | b[0]);
    const uint64_t hi = ((uint64_t)a[3] << 32 | a[2]) + ((uint64_t)b[3] << 32 | b[2]);
    a[0] = (uint32_t)lo;
    a[1] = (uint32_t)(lo >> 32);
    a[2] = (uint32_t)hi;
    a[3] = (uint32_t)(hi >> 32);
}

__device__ __forceinline__ void xor4(uint32_t (&a)[4], const uint32_t (&b)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c)
        a[c] ^= b[c];
}

template <uint32_t NC, int J>
__device__ __forceinline__ void mix_reg(uint32_t (&x)[8][4], const uint32_t (&i1)[4], const uint32_t (&i2)[4], const uint32_t (&i3)[4],
                                        const uint32_t (&i4)[4], const uint32_t* tb)
{
    constexpr int R1 = J & 7, R2 = (J + 4) & 7, R3 = (J + 6) & 7, R4 = (J + 1) & 7, R5 = (J + 2) & 7;
    aesdec4<NC>(x[R1], x[R2], tb);
    paddq4(x[R3], i1);
    xor4(x[R2], i2);
    aesdec4<NC>(x[R2], x[R4], tb);
    paddq4(x[R5], i3);
    xor4(x[R4], i4);
}

template <uint32_t NC, int J>
__device__ __forceinline__ void mix_lane(uint32_t (&x)[8][4], const uint32_t (&L)[8], const uint32_t* tb)
{
    uint32_t i1[4], i2[4], i3[4], i4[4];
    lane_sel<15>(i1, L);
    lane_sel<0>(i2, L);
    lane_sel<1>(i3, L);
    lane_sel<16>(i4, L);
    mix_reg<NC, J>(x, i1, i2, i3, i4, tb);
}

template <uint32_t NC, int I>
__device__ __forceinline__ void shuffle4(uint32_t (&x)[8][4], const uint32_t* tb)
{
    constexpr int R1 = I & 7, R2 = (I + 1) & 7, R3 = (I + 2) & 7, R4 = (I + 4) & 7, R5 = (I + 5) & 7, R6 = (I + 6) & 7;
    aesdec4<NC>(x[R1], x[R4], tb);
    paddq4(x[R2], x[R5]);
    xor4(x[R4], x[R6]);
    aesdec4<NC>(x[R4], x[R2], tb);
    paddq4(x[R5], x[R6]);
    xor4(x[R2], x[R3]);
}

// raw dwords q[d0 .. d0 + N) (the last only when misaligned) of a range's bytes, every one holding a byte of the range (full) or
// read only when it does (d < nd); zero otherwise
template <int N>
__device__ __forceinline__ void load_raw(uint32_t (&w)[N], const uint32_t* q, uint32_t d0, uint32_t nd, uint32_t mis, bool full)
{
    if (full)
    {
#pragma unroll
        for (int i = 0; i + 4 <= N - 1; i += 4)
        {
            const u32x4_a4 v = *reinterpret_cast<const u32x4_a4*>(q + d0 + i);
            w[i] = v.x;
            w[i + 1] = v.y;
            w[i + 2] = v.z;
            w[i + 3] = v.w;
        }
        w[N - 1] = mis ? q[d0 + N - 1] : 0u;
    }
    else
    {
#pragma unroll
        for (int i = 0; i < N; ++i)
            w[i] = d0 + (uint32_t)i < nd ? q[d0 + i] : 0u;
    }
}

// lane k (0..3) of a half-block of raw dwords: its 8 aligned dwords
__device__ __forceinline__ void lane_of(uint32_t (&L)[8], const uint32_t (&w)[33], int k, uint32_t sh)
{
#pragma unroll
    for (int i = 0; i < 8; ++i)
        L[i] = __builtin_amdgcn_alignbit(w[8 * k + i + 1], w[8 * k + i], sh);
}

template <int J0>
__device__ __forceinline__ void mix_half(uint32_t (&x)[8][4], const uint32_t (&w)[33], uint32_t sh, const uint32_t* tb)
{
    uint32_t L[8];
    lane_of(L, w, 0, sh);
    mix_lane<32, J0>(x, L, tb);
    lane_of(L, w, 1, sh);
    mix_lane<32, J0 + 1>(x, L, tb);
    lane_of(L, w, 2, sh);
    mix_lane<32, J0 + 2>(x, L, tb);
    lane_of(L, w, 3, sh);
    mix_lane<32, J0 + 3>(x, L, tb);
}

// the 32-byte lane at byte `at` of the range, bytes at or beyond len zero (reads only the dwords that hold a byte of the range)
__device__ __forceinline__ void load_lane(uint32_t (&L)[8], const uint32_t* q, uint32_t at, uint32_t len, uint32_t nd, uint32_t sh)
{
    uint32_t w[9];
    load_raw<9>(w, q, at >> 2, nd, sh, false);
#pragma unroll
    for (int i = 0; i < 8; ++i)
    {
        uint32_t v = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
        const int64_t rem = (int64_t)len - (int64_t)(at + 4u * (uint32_t)i);
        if (rem <= 0)
            v = 0u;
        else if (rem < 4)
            v &= (1u << (8 * rem)) - 1u;
        L[i] = v;
    }
}

template <int K>
__device__ __forceinline__ void end_lane(uint32_t (&x)[8][4], const uint32_t* q, uint32_t rb, uint32_t cnt, uint32_t len, uint32_t nd,
                                         uint32_t sh, const uint32_t* tb)
{
    if ((uint32_t)K < cnt)
    {
        uint32_t L[8];
        load_lane(L, q, rb + 32u * K, len, nd, sh);
        mix_lane<32, K + 2>(x, L, tb);
    }
}

__global__ __launch_bounds__(256) void k_meow_lanes(const uint8_t* __restrict__ data, const uint64_t* __restrict__ offsets,
                                                    const uint32_t* __restrict__ lens, uint64_t bound, const uint32_t* __restrict__ n_dev,
                                                    const uint32_t* __restrict__ order, const uint32_t* __restrict__ skip,
                                                    uint64_t* __restrict__ hashes)
{
    __shared__ uint32_t s_td[256 * 32];
    const uint32_t* tb = meow_table<32>(s_td);
    const uint32_t n = range_count(bound, n_dev);
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n || (skip && g < *skip)) // (the first *skip ranges of the order are the long ones: k_meow_quads)
        return;
    const uint32_t c = order ? order[g] : (uint32_t)g;
    const uint32_t len = lens[c];
    const uint8_t* p = data + offsets[c];
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t sh = mis * 8u;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - mis);
    const uint32_t nd = len ? (mis + len + 3u) >> 2 : 0u; // raw dwords that hold a byte of the range
    const uint32_t nblocks = len >> 8;

    uint32_t x[8][4];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            x[r][k] = seed_col((uint32_t)r, (uint32_t)k);

    // whole blocks: two half-blocks of 33 raw dwords, one in flight while the other mixes (every dword holds a byte of the range:
    // the spill dword of a misaligned half ends before its last byte)
    uint32_t wa[33], wb[33];
    if (nblocks)
        load_raw<33>(wa, q, 0u, nd, mis, true);
    for (uint32_t b = 0; b < nblocks; ++b)
    {
        load_raw<33>(wb, q, b * 64u + 32u, nd, mis, true);
        mix_half<0>(x, wa, sh, tb);
        if (b + 1u < nblocks)
            load_raw<33>(wa, q, (b + 1u) * 64u, nd, mis, true);
        mix_half<4>(x, wb, sh, tb);
    }

    // MeowEnd
    const uint32_t rb = nblocks * 256u; // the residual: bytes rb .. len
    const uint32_t cnt = (len >> 5) & 7u;
    {
        uint32_t T[8], i1[4], i2[4], i3[4], i4[4];
        load_lane(T, q, rb + cnt * 32u, len, nd, sh);
        lane_sel<31>(i1, T);
        lane_sel<0>(i2, T);
        lane_sel<17>(i3, T);
        lane_sel<16>(i4, T);
        mix_reg<32, 0>(x, i1, i2, i3, i4, tb);
        const uint32_t z[4] = {0u, 0u, 0u, 0u};
        const uint32_t l8[4] = {len >> 8, 0u, 0u, 0u};
        const uint32_t l0[4] = {len, 0u, 0u, 0u};
        mix_reg<32, 1>(x, z, z, l8, l0, tb);
    }
    end_lane<0>(x, q, rb, cnt, len, nd, sh, tb);
    end_lane<1>(x, q, rb, cnt, len, nd, sh, tb);
    end_lane<2>(x, q, rb, cnt, len, nd, sh, tb);
    end_lane<3>(x, q, rb, cnt, len, nd, sh, tb);
    end_lane<4>(x, q, rb, cnt, len, nd, sh, tb);
    end_lane<5>(x, q, rb, cnt, len, nd, sh, tb);
    end_lane<6>(x, q, rb, cnt, len, nd, sh, tb);
    shuffle4<32, 0>(x, tb);
    shuffle4<32, 1>(x, tb);
    shuffle4<32, 2>(x, tb);
    shuffle4<32, 3>(x, tb);
    shuffle4<32, 4>(x, tb);
    shuffle4<32, 5>(x, tb);
    shuffle4<32, 6>(x, tb);
    shuffle4<32, 7>(x, tb);
    shuffle4<32, 0>(x, tb);
    shuffle4<32, 1>(x, tb);
    shuffle4<32, 2>(x, tb);
    shuffle4<32, 3>(x, tb);
    paddq4(x[0], x[2]);
    paddq4(x[1], x[3]);
    paddq4(x[4], x[6]);
    paddq4(x[5], x[7]);
    xor4(x[0], x[1]);
    xor4(x[4], x[5]);
    paddq4(x[0], x[4]);
    hashes[c] = (uint64_t)x[0][0] | ((uint64_t)x[0][1] << 32);
}

// ---------------------------------------------------------------------------------------------------
// quad per message: lane qi of the quad holds x[r] = column qi of register r.  All four lanes of a quad must be active.
// ---------------------------------------------------------------------------------------------------
template <uint32_t NC>
__device__ __forceinline__ uint32_t aesdec_q(uint32_t a, uint32_t k, const uint32_t* tb)
{
    const uint32_t a1 = quad_perm<QP_ROT3>(a); // column c - 1
    const uint32_t a2 = quad_perm<QP_ROT2>(a); // column c - 2
    const uint32_t a3 = quad_perm<QP_ROT1>(a); // column c - 3
    return td<NC, 0>(tb, a & 255u) ^ td<NC, 1>(tb, (a1 >> 8) & 255u) ^ td<NC, 2>(tb, (a2 >> 16) & 255u) ^ td<NC, 3>(tb, a3 >> 24) ^ k;
}

// paddq: the carry of column 0 (2) moves to column 1 (3)
__device__ __forceinline__ uint32_t paddq_q(uint32_t a, uint32_t b, uint32_t qi)
{
    const uint32_t s = a + b;
    const uint32_t cin = quad_perm<QP_ROT3>((uint32_t)(s < a));
    return (qi & 1u) ? s + cin : s;
}

template <uint32_t NC, int J>
__device__ __forceinline__ void mix_reg_q(uint32_t (&x)[8], uint32_t i1, uint32_t i2, uint32_t i3, uint32_t i4, uint32_t qi,
                                          const uint32_t* tb)
{
    constexpr int R1 = J & 7, R2 = (J + 4) & 7, R3 = (J + 6) & 7, R4 = (J + 1) & 7, R5 = (J + 2) & 7;
    x[R1] = aesdec_q<NC>(x[R1], x[R2], tb);
    x[R3] = paddq_q(x[R3], i1, qi);
    x[R2] ^= i2;
    x[R2] = aesdec_q<NC>(x[R2], x[R4], tb);
    x[R5] = paddq_q(x[R5], i3, qi);
    x[R4] ^= i4;
}

// column qi of the 16 bytes at byte O of the 32-byte lane s8 (8 LDS dwords), read cyclically
template <int O>
__device__ __forceinline__ uint32_t lane_sel_q(const uint32_t* s8, uint32_t qi)
{
    const uint32_t d = (uint32_t)(O / 4) + qi;
    return (O & 3) ? __builtin_amdgcn_alignbyte(s8[(d + 1u) & 7u], s8[d & 7u], O & 3) : s8[d & 7u];
}

template <uint32_t NC, int J>
__device__ __forceinline__ void mix_lane_q(uint32_t (&x)[8], const uint32_t* s8, uint32_t qi, const uint32_t* tb)
{
    mix_reg_q<NC, J>(x, lane_sel_q<15>(s8, qi), lane_sel_q<0>(s8, qi), lane_sel_q<1>(s8, qi), lane_sel_q<16>(s8, qi), qi, tb);
}

template <uint32_t NC, int I>
__device__ __forceinline__ void shuffle_q(uint32_t (&x)[8], uint32_t qi, const uint32_t* tb)
{
    constexpr int R1 = I & 7, R2 = (I + 1) & 7, R3 = (I + 2) & 7, R4 = (I + 4) & 7, R5 = (I + 5) & 7, R6 = (I + 6) & 7;
    x[R1] = aesdec_q<NC>(x[R1], x[R4], tb);
    x[R2] = paddq_q(x[R2], x[R5], qi);
    x[R4] ^= x[R6];
    x[R4] = aesdec_q<NC>(x[R4], x[R2], tb);
    x[R5] = paddq_q(x[R5], x[R6], qi);
    x[R2] ^= x[R3];
}

template <uint32_t NC>
__device__ __forceinline__ void block_q(uint32_t (&x)[8], const uint32_t* s, uint32_t qi, const uint32_t* tb)
{
    mix_lane_q<NC, 0>(x, s, qi, tb);
    mix_lane_q<NC, 1>(x, s + 8, qi, tb);
    mix_lane_q<NC, 2>(x, s + 16, qi, tb);
    mix_lane_q<NC, 3>(x, s + 24, qi, tb);
    mix_lane_q<NC, 4>(x, s + 32, qi, tb);
    mix_lane_q<NC, 5>(x, s + 40, qi, tb);
    mix_lane_q<NC, 6>(x, s + 48, qi, tb);
    mix_lane_q<NC, 7>(x, s + 56, qi, tb);
}

template <uint32_t NC, int K>
__device__ __forceinline__ void end_lane_q(uint32_t (&x)[8], const uint32_t* s, uint32_t cnt, uint32_t qi, const uint32_t* tb)
{
    if ((uint32_t)K < cnt) // (uniform per quad)
        mix_lane_q<NC, K + 2>(x, s + 8 * K, qi, tb);
}

// MeowEnd with the residual in s (64 dwords, zero beyond the message) and total length len; returns the digest in lanes 0 (and
// its high half in lane 1)
template <uint32_t NC>
__device__ uint32_t end_q(uint32_t (&x)[8], const uint32_t* s, uint64_t len, uint32_t qi, const uint32_t* tb)
{
    const uint32_t cnt = (uint32_t)(len >> 5) & 7u;
    const uint32_t* t8 = s + 8u * cnt;
    mix_reg_q<NC, 0>(x, lane_sel_q<31>(t8, qi), lane_sel_q<0>(t8, qi), lane_sel_q<17>(t8, qi), lane_sel_q<16>(t8, qi), qi, tb);
    const uint64_t l8 = len >> 8;
    const uint32_t i3 = qi == 0 ? (uint32_t)l8 : qi == 1 ? (uint32_t)(l8 >> 32) : 0u;
    const uint32_t i4 = qi == 0 ? (uint32_t)len : qi == 1 ? (uint32_t)(len >> 32) : 0u;
    mix_reg_q<NC, 1>(x, 0u, 0u, i3, i4, qi, tb);
    end_lane_q<NC, 0>(x, s, cnt, qi, tb);
    end_lane_q<NC, 1>(x, s, cnt, qi, tb);
    end_lane_q<NC, 2>(x, s, cnt, qi, tb);
    end_lane_q<NC, 3>(x, s, cnt, qi, tb);
    end_lane_q<NC, 4>(x, s, cnt, qi, tb);
    end_lane_q<NC, 5>(x, s, cnt, qi, tb);
    end_lane_q<NC, 6>(x, s, cnt, qi, tb);
    shuffle_q<NC, 0>(x, qi, tb);
    shuffle_q<NC, 1>(x, qi, tb);
    shuffle_q<NC, 2>(x, qi, tb);
    shuffle_q<NC, 3>(x, qi, tb);
    shuffle_q<NC, 4>(x, qi, tb);
    shuffle_q<NC, 5>(x, qi, tb);
    shuffle_q<NC, 6>(x, qi, tb);
    shuffle_q<NC, 7>(x, qi, tb);
    shuffle_q<NC, 0>(x, qi, tb);
    shuffle_q<NC, 1>(x, qi, tb);
    shuffle_q<NC, 2>(x, qi, tb);
    shuffle_q<NC, 3>(x, qi, tb);
    const uint32_t a = paddq_q(x[0], x[2], qi) ^ paddq_q(x[1], x[3], qi);
    const uint32_t b = paddq_q(x[4], x[6], qi) ^ paddq_q(x[5], x[7], qi);
    return paddq_q(a, b, qi);
}

__device__ __forceinline__ void quad_seed(uint32_t (&x)[8], uint32_t qi)
{
#pragma unroll
    for (int r = 0; r < 8; ++r)
        x[r] = seed_col((uint32_t)r, qi);
}

// lane qi's 17 raw dwords of the 256-byte block at byte `at` of [p, p + len) (its 16 aligned dwords qi*16 .. +16 and the spill),
// reading only the dwords that hold a byte of it
__device__ __forceinline__ void quad_raw(uint32_t (&w)[17], const uint8_t* p, uint64_t len, uint64_t at, uint32_t qi)
{
    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - mis);
    const uint64_t d0 = at / 4u + qi * 16u;
    const uint64_t nd = len ? (mis + len + 3u) >> 2 : 0u;
#pragma unroll
    for (int i = 0; i < 17; ++i)
        w[i] = d0 + (uint64_t)i < nd && (i < 16 || mis) ? q[d0 + i] : 0u;
}
__device__ __forceinline__ void quad_put(uint32_t* s, const uint32_t (&w)[17], const uint8_t* p, uint64_t len, uint64_t at, uint32_t qi)
{
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u) * 8u;
#pragma unroll
    for (int i = 0; i < 16; ++i)
    {
        uint32_t v = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
        const int64_t rem = (int64_t)len - (int64_t)(at + qi * 64u + 4u * (uint32_t)i);
        if (rem <= 0)
            v = 0u;
        else if (rem < 4)
            v &= (1u << (8 * rem)) - 1u;
        s[qi * 16u + (uint32_t)i] = v;
    }
}

__device__ __forceinline__ void quad_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// absorb the whole blocks of [p, p + len) through the quad's 64 LDS dwords s; final: then MeowEnd over the residual with total
// length t0 + len, the digest returned (lanes 0, 1)
template <uint32_t NC>
__device__ uint32_t chain_q(uint32_t (&x)[8], const uint8_t* p, uint64_t len, uint64_t t0, bool final, uint32_t* s, uint32_t qi,
                            const uint32_t* tb)
{
    const uint64_t nblocks = len >> 8;
    uint32_t w[17];
    quad_raw(w, p, len, 0u, qi);
    for (uint64_t b = 0; b < nblocks; ++b)
    {
        quad_put(s, w, p, len, b * 256u, qi);
        quad_sync();
        quad_raw(w, p, len, (b + 1u) * 256u, qi); // in flight during the mixes (the residual, or nothing, after the last block)
        block_q<NC>(x, s, qi, tb);
        quad_sync();
    }
    if (!final)
        return 0u;
    quad_put(s, w, p, len, nblocks * 256u, qi);
    quad_sync();
    return end_q<NC>(x, s, t0 + len, qi, tb);
}

// a quad per range (16 ranges per 64-lane workgroup): few ranges, or long ones.  order == null: ranges 0 .. n; else the first
// *n_long ranges of the length-class order (the longest), grid-strided
__global__ __launch_bounds__(64) void k_meow_quads(const uint8_t* __restrict__ data, const uint64_t* __restrict__ offsets,
                                                   const uint32_t* __restrict__ lens, uint64_t bound, const uint32_t* __restrict__ n_dev,
                                                   const uint32_t* __restrict__ order, const uint32_t* __restrict__ n_long,
                                                   uint64_t* __restrict__ hashes)
{
    __shared__ uint32_t s_td[256 * 32];
    __shared__ uint32_t s_blk[16 * 64];
    const uint32_t* tb = meow_table<32>(s_td);
    const uint32_t n = order ? *n_long : range_count(bound, n_dev);
    const uint32_t qi = threadIdx.x & 3u;
    uint32_t* s = s_blk + (threadIdx.x >> 2) * 64u;
    for (uint64_t i = (uint64_t)blockIdx.x * 16u + (threadIdx.x >> 2); i < n; i += (uint64_t)gridDim.x * 16u) // (uniform per quad)
    {
        const uint32_t c = order ? order[i] : (uint32_t)i;
        uint32_t x[8];
        quad_seed(x, qi);
        const uint32_t lo = chain_q<32>(x, data + offsets[c], lens[c], 0u, true, s, qi, tb);
        const uint32_t hi = quad_perm<QP_ROT1>(lo);
        if (qi == 0)
            hashes[c] = (uint64_t)lo | ((uint64_t)hi << 32);
    }
}

// ONE input of at most 64 KiB, staged into LDS by the whole wave (stage_input_lds), then hashed by the first quad from LDS
__global__ __launch_bounds__(64) void k_meow_one(const uint8_t* __restrict__ in, uint32_t len, uint64_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_in[]; // the whole blocks and one residual block, zero-padded
    __shared__ uint32_t s_td[256 * 4];
    const uint32_t lane = threadIdx.x;
    const uint32_t nblocks = len >> 8;
    stage_input_lds(s_in, (nblocks + 1u) * 64u, in, len, lane);
    const uint32_t* tb = meow_table<4>(s_td);
    if (lane >= 4u)
        return;
    uint32_t x[8];
    quad_seed(x, lane);
    for (uint32_t b = 0; b < nblocks; ++b)
        block_q<4>(x, s_in + b * 64u, lane, tb);
    const uint32_t lo = end_q<4>(x, s_in + nblocks * 64u, len, lane, tb);
    const uint32_t hi = quad_perm<QP_ROT1>(lo);
    if (lane == 0)
        *out = (uint64_t)lo | ((uint64_t)hi << 32);
}

// Streaming: the state in device memory is {x[8][4], bytes so far (u64)}.  A batch is a run of whole blocks; the final call absorbs the
// rest, ends with the total length and writes the digest.  first: no state yet (the seed).
__global__ __launch_bounds__(64) void k_meow_stream(const uint8_t* __restrict__ data, uint32_t len, uint32_t* __restrict__ state, int first,
                                                    int final, uint64_t* __restrict__ out)
{
    __shared__ uint32_t s_td[256 * 4];
    __shared__ uint32_t s_blk[64];
    const uint32_t* tb = meow_table<4>(s_td);
    const uint32_t qi = threadIdx.x;
    if (qi >= 4u)
        return;
    uint32_t x[8];
    uint64_t t0 = 0;
    if (first)
        quad_seed(x, qi);
    else
    {
#pragma unroll
        for (int r = 0; r < 8; ++r)
            x[r] = state[4 * r + qi];
        t0 = (uint64_t)state[32] | ((uint64_t)state[33] << 32);
    }
    const uint32_t lo = chain_q<4>(x, data, len, t0, final != 0, s_blk, qi, tb);
    if (final)
    {
        const uint32_t hi = quad_perm<QP_ROT1>(lo);
        if (qi == 0)
            *out = (uint64_t)lo | ((uint64_t)hi << 32);
    }
    else
    {
#pragma unroll
        for (int r = 0; r < 8; ++r)
            state[4 * r + qi] = x[r];
        if (qi == 0)
        {
            const uint64_t t = t0 + len;
            state[32] = (uint32_t)t;
            state[33] = (uint32_t)(t >> 32);
        }
    }
}

// the launch policy of k_hash_common.h over the four kernels
struct MeowKind
{
    static constexpr auto lanes = &k_meow_lanes, quads = &k_meow_quads;
    static constexpr auto one = &k_meow_one;
    static constexpr auto stream = &k_meow_stream;
    static constexpr int kid = LTHIP_K_OTHER;
    static constexpr const char* name = "meow";
    static constexpr const char* name_one = "meow_one";
    static constexpr uint32_t unit_shift = 8u;
    static constexpr uint32_t long_class = 12u * 4u; // >= 1 MiB: 4096 blocks of 256 bytes
    static size_t one_lds(uint32_t len) { return (size_t)((len >> 8) + 1u) * 256u; }
    static constexpr size_t one_lds_grant = 64u * 1024u - 8u * 1024u;
};

} // namespace

const ChainHash* lthip_chain_meow()
{
    static const ChainHash kind = {chain_launch_ranges<MeowKind>, chain_launch_one<MeowKind>, chain_launch_stream<MeowKind>, LTHIP_MEOW_STREAM_BATCH};
    return &kind;
}
