// k_buzhash.hip -- content-defined chunking on gfx950.
//
// Reference behaviour: lib/hpcdcchunker/longtail_hpcdcchunker.c (Longtail_HPCDCNextChunk :225-310).
// MI355X formulation:
//   K1 k_buzhash_prefix_dma: H(p) = XOR_{j<48} rotl(T[byte[p-1-j]], j) is a pure function of the 48 bytes before p, so every
//                           position of every part is evaluated independently.  ONE persistent workgroup of 16 waves per CU;
//                           each WAVE owns 4 KiB wave-tiles end to end -- no workgroup barrier in the loop.  The tile comes
//                           straight from global memory into the wave's LDS buffer (global_load_lds_dwordx4), every lane
//                           keeps the SUFFIX XORs of its own 64-byte run in registers (prefix-XOR formulation: one table
//                           look-up per byte, no 48-byte warm-up; the neighbour's suffixes through one v_xor_b32_dpp).
//                           The LDS table holds T[256] in all 32 rotations, R[r][v] = rotr(T[v], r) at byte r * 1024 + v * 4
//                           (32 KiB): the look-up of the byte at run position j reads R[j mod 32] -- the address is ONE SDWA
//                           shift of the data dword (byte << 2), the row is the instruction's offset field, and the word
//                           arrives rotated into the de-rotated frame.  One copy means bank = v mod 32: look-ups of
//                           different bytes can conflict (random bytes: ~3.2 LDS cycles per 32 lanes instead of 1, at
//                           most 8), which the LDS array has the room for; the rotate they save was a VALU instruction
//                           per byte of an issue-bound kernel (profiles/buzhash_rot_table_ab.txt).
//                           `H % d == d-1` is a necessary test on the odd part of d accumulated over eight steps, the exact
//                           multiply-add + rotate + compare only in the rare wave-uniform branch.  Output is a two level
//                           bitmap: level 0 one bit per byte (only non-zero words are stored), level 1 one bit per 64-byte
//                           run (wave ballot, always stored).  (Earlier formulations -- the rolling-window kernel of
//                           rounds 1-2, register staging -- live in ablations/ and are compiled by `make ablations` only.)
//   K2 select_cuts        : one wave per part walks chunk by chunk: wave-wide load of the level-1 words that
//                           cover (start+min, start+max], first flagged run, one level-0 word, ffs.
//   K3 compact            : scan of per-part counts, gather into dense (offset,len) arrays.
#include "lthip_internal.h"

#include <stdlib.h>
#include <type_traits>

namespace
{

__constant__ uint32_t c_buztab[256] = {
#include "buzhash_table.inc"
};

#include "k_blake3_leaf.h" // the hashing of one BLAKE3 leaf in a lane's registers (k_buzhash_hash_walk)

constexpr int RUN = 64;                      // bytes per thread
constexpr int TILE = 256 * RUN;              // 16 KiB: the plan's tile (four wave-tiles)
constexpr int ROW_DW = 17;                   // 16 data dwords + 1 pad: thread-strided ds_read_b32 hits 32 distinct banks
constexpr int TAB_ROT = 32;                  // the table holds every rotation: R[r][v] = rotr(T[v], r) at LDS dword r * 256 + v
constexpr int TAB_DW = TAB_ROT * 256;        // 32 KiB, one copy: bank = v mod 32, so a look-up can conflict (at most 8 values a bank)

// 32-bit load from a raw LDS byte address (the device pass only: LDS pointers are 32 bits wide there)
__device__ __forceinline__ uint32_t lds_load_u32(uint32_t byte_addr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(3))) uint32_t*)byte_addr;
#else
    (void)byte_addr;
    return 0u;
#endif
}

__device__ __forceinline__ uint32_t lds_load_u8(uint32_t byte_addr)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(3))) uint8_t*)byte_addr;
#else
    (void)byte_addr;
    return 0u;
#endif
}

__device__ __forceinline__ uint4 lds_load_u128(uint32_t byte_addr) // 16-byte aligned: ONE ds_read_b128
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    const v4 q = *(const __attribute__((address_space(3))) v4*)byte_addr;
    return make_uint4(q.x, q.y, q.z, q.w);
#else
    (void)byte_addr;
    return make_uint4(0, 0, 0, 0);
#endif
}

__device__ __forceinline__ uint32_t rotl32(uint32_t x, uint32_t r) { return __builtin_amdgcn_alignbit(x, x, (32u - r) & 31u); }
__device__ __forceinline__ uint32_t rotr32(uint32_t x, uint32_t r) { return __builtin_amdgcn_alignbit(x, x, r & 31u); }

// ---------------------------------------------------------------------------------------------------
// tile -> part table (built once per plan)
// ---------------------------------------------------------------------------------------------------
__global__ void k_tile_table(const PartDev* __restrict__ parts, uint32_t nparts, uint32_t* __restrict__ tile_part,
                             uint64_t ntiles)
{
    uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles)
        return;
    // last part whose tile_base <= t and that owns at least one tile
    uint32_t lo = 0, hi = nparts; // invariant: parts[lo].tile_base <= t
    while (hi - lo > 1)
    {
        uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)parts[mid].tile_base <= t)
            lo = mid;
        else
            hi = mid;
    }
    tile_part[t] = lo; // empty parts share their tile_base with the next part; the search lands on the last one (non-empty)
}

// ---------------------------------------------------------------------------------------------------
// K1
// ---------------------------------------------------------------------------------------------------
// The unit of work is a WAVE-tile: 4 KiB of one part (+64 B halo in front) staged into the wave's private LDS
// rows; waves of a workgroup share nothing but the read-only table, so there is no barrier in the loop.  The loads
// of the next wave-tile are issued before the current one is hashed (register double buffering).
constexpr int WROWS = 64 + 1;            // 64 data rows + 1 halo row
constexpr int WTILE = 64 * RUN;          // 4 KiB

#ifdef LTHIP_ABLATIONS
#include "ablations/k_buzhash_roll.inc"
#endif

// ---------------------------------------------------------------------------------------------------
// K1, prefix-XOR formulation (round 3; the default).
//
// In the de-rotated frame U[q] = rotr(T[b_q], q mod 32) the window hash of hpcdcchunker.c:266-306 is
//     H(p) = rotl( XOR_{q=p-48}^{p-1} U[q], (p-1) mod 32 )
// (rotl(U[p-1-j], p-1) = rotl(T[b_{p-1-j}], j)), so a lane that owns the 64-byte aligned run [q0, q0+64) needs ONE table
// look-up per byte and no 48-byte warm-up: with the suffix XORs S[k] = XOR_{i>=k} U[q0+i] (S[64] = 0) of its own run,
//     k >= 47:  W = S[k-47] ^ S[k+1]                                  (window inside the run)
//     k <  47:  W = S[0] ^ S[k+1] ^ S'[k+17]                          (S' = the suffix XORs of the run before = lane-1:
//                                                                      one v_xor_b32_dpp wave_ror:1)
//     H(q0+k+1) = rotl(W, k mod 32)                                   (compile-time rotate: q0 is a multiple of 64)
// Lane 0's predecessor is the halo row: its 47 suffix XORs are made by the whole wave (one byte per lane, wave scan),
// parked in LDS, and loaded into LANE 63's registers S[17..63] once that lane has used them itself -- the steps run from
// k = 63 down, so a register's own use (step j-1) precedes its use by the neighbour (step j-17) -- where wave_ror:1
// hands them to lane 0.  The cut test is accumulated: y = H*inv + inv (<= qodd iff the odd part of d divides H+1) of
// eight steps goes through v_min3_u32, one compare and one scalar branch per eight bytes; the exact test only in the
// rare branch.  U[q] is not computed: q0 is a multiple of 64 in the tile's frame, so the rotation of the byte at run position j is the
// constant j mod 32, and the LDS table holds T in all 32 rotations, R[r][v] = rotr(T[v], r) at byte r * 1024 + v * 4 -- the
// look-up's address is byte << 2 (one SDWA shift of the data dword), its row the offset field of the ds_read_b32, and pass A is
// one XOR per byte.  (A tile of the walking scans starts at a multiple of 16 of its part, not of 64: the frame is the tile's, and
// H comes out the same, since rotl(U[p-1-j], p-1) = rotl(T[b], j) whatever q0 is counted from.)
// ~7.4 VALU instructions per byte and lane (8.4 with the rotate of the look-up in pass A, 11.5 for the rolling window), 64 + 16
// live values instead of 112 + 28.
// ---------------------------------------------------------------------------------------------------
#ifndef K1_MAD64
#define K1_MAD64 0 // measured: 5.88 against 5.76 ms per 16 GiB -- not kept
#endif
constexpr int HALO_DW = 64; // per wave: suffix XORs of the halo row, dword j = S'[j]

struct PrefixConsts
{
    uint32_t hj;        // the halo byte this lane looks up (63 - lane)
    uint32_t halo_byte; // LDS byte address of the wave's halo[] array
    uint32_t thr;       // y <= thr is necessary for a cut
    uint32_t exact_add; // H*inv + addc = y + exact_add
};

// LDS byte address of R[j mod 32][byte j of the run]: byte << 2 is ONE SDWA shift of the data dword (left to the compiler, byte 0 of
// a dword costs a shift and an and), the row is a constant that the load takes into its offset field
// (j is a constant of the caller's unrolled loop)
__device__ __forceinline__ uint32_t prefix_lookup(uint32_t w, int j)
{
    uint32_t a = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#define LT_BYTE4(n) asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_" #n : "=v"(a) : "v"(w))
    if ((j & 3) == 0)
        LT_BYTE4(0);
    else if ((j & 3) == 1)
        LT_BYTE4(1);
    else if ((j & 3) == 2)
        LT_BYTE4(2);
    else
        LT_BYTE4(3);
#undef LT_BYTE4
#else
    (void)w;
#endif
    return lds_load_u32(a + (uint32_t)(j & 31) * 1024u);
}

// One wave-tile: win[] = the lane's own 64-byte run, hb = the lane's halo byte (byte 63 - lane of the 64 bytes before the
// tile; lanes >= 47 are ignored).  Returns the 64 candidate bits of the run, bit k <=> cut position q0 + k + 1.
template <int MODE>
__device__ __forceinline__ uint64_t prefix_tile(const uint32_t (&win)[16], uint32_t hb, const PrefixConsts& pc, const DivTest& dv,
                                                int lane, uint32_t* __restrict__ halo)
{
    // ---- halo: S'[j] for j = 17..63 by a wave scan, to LDS ----
    {
        uint32_t x = lds_load_u32(((pc.hj & 31u) << 10) + (hb << 2)); // R[hj mod 32][hb]
        if (lane >= 47)
            x = 0u;
        // inclusive XOR scan over the lanes: lane i gets the bytes 63-i .. 63 = S'[63 - i]
        x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false); // row_shr:1
        x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false); // row_shr:2
        x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false); // row_shr:4
        x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false); // row_shr:8
        x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false); // row_bcast:15
        x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false); // row_bcast:31
        halo[pc.hj] = x;
    }

    // ---- pass A: suffix XORs of the lane's own run ----
    uint32_t S[65];
#pragma unroll
    for (int j = 63; j >= 0; --j)
        S[j] = prefix_lookup(win[j >> 2], j); // R[j mod 32][b_j] = U[q0 + j]
    __builtin_amdgcn_sched_barrier(0);
    S[64] = 0u;
#pragma unroll
    for (int j = 63; j >= 0; --j)
        S[j] ^= S[j + 1]; // the words come rotated: no rotate here
    __builtin_amdgcn_wave_barrier(); // halo[] written by all lanes, read by lane 63 below

    // ---- pass B: eight steps per group, from the top ----
    // Lane 63 hands the halo's suffixes to lane 0 (wave_ror:1): once the steps down to k = 4n are done, lane 63 has used
    // S[4n+4 .. 4n+7] for the last time (own use of S[j]: step j - 1), and the neighbour steps that read them (k = j - 17 =
    // 4n-13 .. 4n-10) lie two to three half-groups ahead: lane 63 takes the halo's values there with one exec-masked
    // ds_read_b128 per half-group, written by hand -- the compiler's version of `if (lane == 63) S[j] = halo[j]` waits for
    // the LDS right behind the branch; here the wait (lgkmcnt counts: LDS operations complete in order) sits in front of the
    // half-group that reads them, with the two younger loads still in flight.
    uint32_t mlo = 0, mhi = 0;
    uint32_t inv_v; // the addend in a VGPR: v_add_u32 with two VGPR sources issues at the double rate, with an SGPR source it does not
    asm volatile("v_mov_b32 %0, %1" : "=v"(inv_v) : "s"(dv.inv));
#if K1_MAD64
    const uint64_t inv64 = (uint64_t)inv_v;
#endif
    // A register that an asm load is still writing must not be touched by anything the compiler generates (a copy made
    // between the load and its wait reads the OLD value whenever the data has not landed: a rare, timing-dependent wrong
    // hand-off -- seen with the tuple taken apart right behind the load).  So a quad stays ONE 128-bit value from the load
    // statement to the wait statement, both tie it in and out, and it is taken apart only behind the wait.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 Q[16];
    auto halo_quad = [&](auto QI) __attribute__((always_inline)) // lane 63: quad q = halo[4q .. 4q+3], issued
    {
        constexpr int q = decltype(QI)::value;
        if constexpr (q >= 4 && q <= 15)
        {
            u32x4 v = {S[4 * q], S[4 * q + 1], S[4 * q + 2], S[4 * q + 3]};
            uint64_t save;
            asm volatile("s_mov_b64 %[sv], exec\n\ts_mov_b64 exec, %[msk]\n\t"
                         "ds_read_b128 %[r], %[ad] offset:%[o]\n\t"
                         "s_mov_b64 exec, %[sv]"
                         : [sv] "=&s"(save), [r] "+v"(v)
                         : [ad] "v"(pc.halo_byte), [msk] "s"(0x8000000000000000ull), [o] "i"(16 * q)
                         : "memory"); // reads halo[]: the store above may not sink below it
            Q[q] = v;
        }
    };
    auto halo_wait = [&](auto QI) __attribute__((always_inline)) // in front of the first half-group that reads quad q through the DPP
    {
        constexpr int q = decltype(QI)::value;
        if constexpr (q >= 4 && q <= 15)
        {
            // younger loads still in flight: those of the (at most two) half-groups executed since quad q was issued
            u32x4 v = Q[q];
            if constexpr (q >= 6)
                asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(v));
            else if constexpr (q == 5)
                asm volatile("s_waitcnt lgkmcnt(1)" : "+v"(v));
            else
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v));
            S[4 * q] = v.x;
            S[4 * q + 1] = v.y;
            S[4 * q + 2] = v.z;
            S[4 * q + 3] = v.w;
        }
    };
    auto group = [&](auto G) __attribute__((always_inline))
    {
        constexpr int g = decltype(G)::value;
        uint32_t y[8];
#pragma unroll
        for (int half = 1; half >= 0; --half)
        {
            // steps 8g + 4 half + 3 .. 8g + 4 half =: 4n + 3 .. 4n read, through the DPP, S[4n+17 .. 4n+20]: quads n+4 and n+5
            // (S[4n+20], the first register of quad n+5, was waited for by half-group n+1, which ran before this one)
            if (half == 1)
                halo_wait(std::integral_constant<int, 2 * g + 1 + 4>{});
            else
                halo_wait(std::integral_constant<int, 2 * g + 4>{});
#pragma unroll
            for (int ii = 3; ii >= 0; --ii)
            {
                const int i = 4 * half + ii;
                const int k = 8 * g + i;
                uint32_t w;
                if (k >= 47)
                    w = S[k - 47] ^ S[k + 1];
                else
                    w = (S[0] ^ S[k + 1]) ^ (uint32_t)__builtin_amdgcn_update_dpp(0, (int)S[(k + 17) & 63], 0x13C, 0xf, 0xf, false); // wave_ror:1
                const uint32_t h = (k & 31) ? rotl32(w, (uint32_t)(k & 31)) : w;
                if (MODE == 1)
                    y[i] = ~h & (dv.d - 1u);
                else
                {
#if K1_MAD64
                    // h * inv + inv in ONE instruction (measured 5.3 cycles against 4.2 + 2.8 for v_mul_lo_u32 + v_add_u32); the
                    // upper half of the 64-bit result and the carry are not used
                    uint64_t t, carry;
                    asm("v_mad_u64_u32 %0, %1, %2, %3, %4" : "=v"(t), "=s"(carry) : "v"(h), "s"(dv.inv), "v"(inv64));
                    y[i] = (uint32_t)t;
#else
                    y[i] = h * dv.inv + inv_v;
#endif
                }
            }
            // steps down to 4n are done: quad n + 1
            if (half == 1)
                halo_quad(std::integral_constant<int, 2 * g + 2>{});
            else
                halo_quad(std::integral_constant<int, 2 * g + 1>{});
        }
        const uint32_t m = min(min(min(y[0], y[1]), y[2]), min(min(min(y[3], y[4]), y[5]), min(y[6], y[7])));
        if (__builtin_amdgcn_ballot_w64(m <= pc.thr) != 0ull) // wave-uniform, one group in ~6
        {
            asm volatile("");
#pragma unroll
            for (int i = 0; i < 8; ++i)
            {
                const int k = 8 * g + i;
                if (__builtin_amdgcn_ballot_w64(y[i] <= pc.thr) != 0ull)
                {
                    asm volatile("");
                    const bool hit = MODE == 1 ? y[i] == 0u : rotr32(y[i] + pc.exact_add, dv.k2) <= dv.qlim; // h % d == d-1
                    uint32_t hbit;
                    asm volatile("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(hbit) : "s"(__builtin_amdgcn_ballot_w64(hit)));
                    if (k < 32)
                        mlo |= hbit << k;
                    else
                        mhi |= hbit << (k - 32);
                }
            }
        }
    };
    group(std::integral_constant<int, 7>{});
    group(std::integral_constant<int, 6>{});
    group(std::integral_constant<int, 5>{});
    group(std::integral_constant<int, 4>{});
    group(std::integral_constant<int, 3>{});
    group(std::integral_constant<int, 2>{});
    group(std::integral_constant<int, 1>{});
    group(std::integral_constant<int, 0>{});
    return ((uint64_t)mhi << 32) | mlo;
}

// candidate bits of a run -> the legal ones (cuts p with 48 <= p <= size), 0 for runs beyond the part
__device__ __forceinline__ uint64_t prefix_legal(uint64_t m, uint64_t q0, uint64_t size)
{
    if (q0 >= size)
        return 0ull;
    if (q0 < 47)
        m &= ~0ull << (47 - q0);
    const uint64_t remain = size - q0; // >= 1
    if (remain < 64)
        m &= (1ull << remain) - 1ull;
    return m;
}

__device__ __forceinline__ void prefix_table_init(uint32_t* tab, int tid, int nthreads)
{
    for (int i = tid; i < TAB_DW; i += nthreads) // R[r][v] = rotr(T[v], r) at dword r * 256 + v
        tab[i] = rotr32(c_buztab[i & 255], (uint32_t)i >> 8);
    __syncthreads(); // the only barrier: table visible to every wave
    if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)tab != 0u)
        __builtin_trap(); // a look-up address is byte * 4 plus the row in the offset field: no base add
}

#ifdef LTHIP_ABLATIONS
#include "ablations/k_buzhash_prefix_regs.inc"
#endif

// Flavour 2 (default): the wave-tile comes straight from global memory into LDS (global_load_lds_dwordx4, 1 KiB per
// instruction, no staging registers and no ds_write pass).  The LDS image of an LDS-DMA is lane-linear (base + instruction
// offset + lane * 16), so the rows cannot be padded; the bank spread comes from the SOURCE side instead: the wave's buffer holds
// 65 rows x 4 vectors of 16 bytes (row 0 = the 64 bytes before the tile), and slot (r, c') receives data vector
// c = c' ^ ((r >> 2) & 3) of row r -- lane L then reads its row r = L + 1 with four ds_read_b128 at slots c ^ ((r >> 2) & 3),
// which puts the sixteen lanes of every ds_read_b128 service group on sixteen different 16-byte slots (checked for all four
// groups).  ONE buffer per wave: the run is in registers after the four reads, so the next tile's DMA is issued right behind
// them and has the whole hashing of this tile to land; the results of a tile are stored at the start of the NEXT iteration,
// in front of that issue, so that the vmcnt(0) which retires the DMA never waits for a store just issued.
constexpr int DMA_BUF_B = WROWS * 64; // 4160 bytes, linear

// The dynamic LDS of the kernels fed by LDS-DMA, in dwords: the table, then per wave its tile buffer and its halo[]; behind them, in the
// walking scan that hashes, per wave a pending list of PEND_CAP chunks (uint4 each).  Kernels and launchers read the layout from here.
constexpr int DMA_WAVE_DW = (DMA_BUF_B >> 2) + HALO_DW;
constexpr int PEND_CAP = 64;
constexpr size_t lds_tiles_dw(int waves) { return TAB_DW + (size_t)waves * DMA_WAVE_DW; }
constexpr size_t lds_pend_dw(int waves) { return lds_tiles_dw(waves); } // where the lists start
constexpr size_t lds_bytes(int waves, bool lists) { return sizeof(uint32_t) * lds_pend_dw(waves) + (lists ? sizeof(uint4) * waves * PEND_CAP : 0); }

struct WaveLds
{
    uint32_t* buf;  // the wave's tile buffer (TileDma)
    uint32_t* halo; // HALO_DW dwords behind it
    uint4* pend;    // the wave's pending list: there only if the launch asked for lds_bytes(WAVES, true)
};
template <int WAVES>
__device__ __forceinline__ WaveLds wave_lds(uint32_t* smem, int wave)
{
    uint32_t* buf = smem + TAB_DW + wave * DMA_WAVE_DW;
    return {buf, buf + (DMA_BUF_B >> 2), reinterpret_cast<uint4*>(smem + lds_pend_dw(WAVES)) + wave * PEND_CAP};
}

// The LDS-DMA staging of one wave: its buffer, the lane's place in a DMA instruction and in the buffer, and the issue of a wave-tile.
struct TileDma
{
    const uint8_t* data;
    uint32_t* buf;
    int lane;
    uint32_t buf_byte; // LDS byte address of the buffer
    uint32_t buf_mid;  // M0 (the LDS base of an LDS-DMA) points at the MIDDLE of the buffer for the whole kernel, the five pieces are told
                       // apart by the instruction offset (13 bits, signed: -2048 .. +2048), which the hardware adds to the LDS address and
                       // to the global address alike
    uint32_t src_off;  // byte offset of the lane's source vector inside a 1 KiB piece
    uint32_t own_row;  // own row r = lane + 1: data vector c sits at slot c ^ own_f, own_f = (r >> 2) & 3
    uint32_t own_f;

    __device__ __forceinline__ TileDma(const uint8_t* d, uint32_t* b, int ln) : data(d), buf(b), lane(ln)
    {
        buf_byte = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)buf);
        buf_mid = buf_byte + 2048u;
        // DMA instruction u moves vector V = 64 u + lane = slot (r = V >> 2, c' = V & 3); (r >> 2) & 3 = (lane >> 4) & 3 for every u
        const uint32_t src_vec = 4u * ((uint32_t)lane >> 2) + (((uint32_t)lane & 3u) ^ (((uint32_t)lane >> 4) & 3u));
        src_off = 16u * src_vec;
        own_f = (((uint32_t)lane + 1u) >> 2) & 3u;
        own_row = buf_byte + 64u * ((uint32_t)lane + 1u);
    }

    template <int MODE>
    __device__ __forceinline__ PrefixConsts consts(const DivTest& dv) const
    {
        PrefixConsts pc;
        pc.hj = 63u - (uint32_t)lane;
        pc.halo_byte = buf_byte + DMA_BUF_B;
        pc.thr = MODE == 1 ? 0u : 0xFFFFFFFFu / (dv.d >> dv.k2);
        pc.exact_add = dv.addc - dv.inv;
        return pc;
    }

    template <int u>
    __device__ __forceinline__ void piece(const uint8_t* mid_src) const
    {
        asm volatile("s_mov_b32 m0, %[l]\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %[v], %[b] offset:%[o]"
                     :
                     : [v] "v"(src_off), [l] "s"(buf_mid), [b] "s"(mid_src), [o] "i"(1024 * u - 2048)
                     : "memory");
    }

    // a tile at an end of its part: vectors outside the part are not loaded (the slot keeps stale bytes; every position they could
    // influence is masked by the caller), the vector that straddles the end is assembled from byte loads and stored by its lane
    template <int u>
    __device__ __forceinline__ void edge(const PartDev& p, uint64_t sp, const uint8_t* mid_src) const
    {
        // The lane's vector lies at part-relative base + src_off.  base (>= -64) is wave-uniform, so where the part begins and ends is
        // two scalars relative to it and the lane's tests are 32-bit against its src_off (a multiple of 16, <= 1008): no lane holds a
        // 64-bit position or address (held across the whole tile loop for all five pieces, they were 30 registers of the walking scan)
        const int64_t base = (int64_t)sp - 64 + 1024 * u;
        const int64_t left = (int64_t)p.size - base;                                      // bytes from base to the part's end: |left| < 2^33
        const int32_t left_hi = (int32_t)(left >> 32);
        const uint32_t before = base < 0 ? (uint32_t)-base : 0u;                          // bytes of the piece in front of the part
        const uint32_t room = left_hi < 0 ? 0u : left_hi > 0 || (uint32_t)left > 1024u ? 1024u : (uint32_t)left;
        const uint32_t room16 = room & ~15u;                                              // the vectors below it lie inside the part
        const bool lane_on = (u < 4 || lane < 4) && src_off >= before;
        const bool whole = lane_on && src_off < room16;
        const bool part = lane_on && src_off == room16 && room != room16;                 // the vector that straddles the end
        if (whole)
            piece<u>(mid_src);
        if (part)
        {
            const uint8_t* src = mid_src + (1024 * u - 2048); // the piece's first byte
            uint32_t w[4] = {0, 0, 0, 0};
            const uint32_t n = room - src_off;
            for (uint32_t bb = 0; bb < n; ++bb)
                w[bb >> 2] |= (uint32_t)src[src_off + bb] << (8 * (bb & 3));
            uint32_t* d = buf + 256 * u + 4 * lane;
            d[0] = w[0];
            d[1] = w[1];
            d[2] = w[2];
            d[3] = w[3];
        }
    }

    // issue the DMA of the wave-tile at part-relative `sp` (a multiple of 16) of part `p` into the wave's buffer
    __device__ __forceinline__ void issue(const PartDev& p, uint64_t sp) const
    {
        const uint8_t* mid_src = data + p.off + sp - 64 + 2048; // the source of the buffer's middle (sp == 0: row 0 lies before the part and is not loaded)
        if (sp >= 64 && sp + (uint64_t)WTILE <= p.size) // every vector inside the part: the common case
        {
            asm volatile("s_mov_b32 m0, %[l]\n\ts_nop 0\n\t"
                         "global_load_lds_dwordx4 %[v], %[b] offset:-2048\n\t"
                         "global_load_lds_dwordx4 %[v], %[b] offset:-1024\n\t"
                         "global_load_lds_dwordx4 %[v], %[b] offset:0\n\t"
                         "global_load_lds_dwordx4 %[v], %[b] offset:1024"
                         :
                         : [v] "v"(src_off), [l] "s"(buf_mid), [b] "s"(mid_src)
                         : "memory");
            if (lane < 4) // vectors 256..259: row 64 (src_off = 16 * lane for these lanes)
                piece<4>(mid_src);
        }
        else
        {
            edge<0>(p, sp, mid_src);
            edge<1>(p, sp, mid_src);
            edge<2>(p, sp, mid_src);
            edge<3>(p, sp, mid_src);
            edge<4>(p, sp, mid_src);
        }
    }

    // the landed tile into registers: win[] = the lane's 64-byte run, hb = its halo byte; the buffer is free on return
    __device__ __forceinline__ void take(uint32_t (&win)[16], uint32_t& hb, const PrefixConsts& pc) const
    {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the tile has landed (and the stores issued before it are done)
#pragma unroll
        for (int c = 0; c < 4; ++c)
        {
            const uint4 q = lds_load_u128(own_row + 16u * ((uint32_t)c ^ own_f));
            win[4 * c + 0] = q.x;
            win[4 * c + 1] = q.y;
            win[4 * c + 2] = q.z;
            win[4 * c + 3] = q.w;
        }
        hb = lds_load_u8(buf_byte + pc.hj); // row 0 = the halo row, f(0) = 0
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
};

// the level-0 words of a wave-tile as a SCALAR base, to be indexed by the lane's 32-bit number: left to itself the compiler keeps
// bm0 + lane in a 64-bit register pair for the whole tile loop
__device__ __forceinline__ uint64_t* run_words(uint64_t* __restrict__ bm0, uint64_t first)
{
    uint64_t* w = bm0 + first;
    asm("" : "+s"(w));
    return w;
}

template <int MODE, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_buzhash_prefix_dma(const uint8_t* __restrict__ data,
                                                                       const PartDev* __restrict__ parts,
                                                                       const uint32_t* __restrict__ tile_part,
                                                                       uint32_t ntiles, DivTest dv,
                                                                       uint64_t* __restrict__ bm0,
                                                                       uint64_t* __restrict__ bm1)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const WaveLds lds = wave_lds<WAVES>(smem, wave);
    uint32_t* const halo = lds.halo;
    prefix_table_init(smem, tid, 64 * WAVES);

    const TileDma dma(data, lds.buf, lane);
    const PrefixConsts pc = dma.consts<MODE>(dv);

    const uint64_t nwt = (uint64_t)ntiles * 4u;
    const uint64_t wstride = (uint64_t)gridDim.x * (uint64_t)WAVES;
    uint64_t wt = (uint64_t)blockIdx.x * (uint64_t)WAVES + (uint64_t)wave;
    if (wt >= nwt)
        return;

    PartDev pd = parts[tile_part[wt >> 2]];
    uint64_t span = ((wt >> 2) - pd.tile_base) * (uint64_t)TILE + (wt & 3u) * (uint64_t)WTILE; // part-relative
    dma.issue(pd, span);

    uint64_t pend_m = 0, pend_summary = 0, pend_i0 = 0, pend_i1 = 0; // results of the tile before, stored one iteration late
    bool pend = false;
    for (;;)
    {
        uint32_t win[16], hb;
        dma.take(win, hb, pc); // (waits for the stores of two tiles ago as well)

        if (pend)
        {
            if (pend_m != 0ull)
                run_words(bm0, pend_i0)[(uint32_t)lane] = pend_m; // one word per 64-byte run
            if (lane == 0)
                bm1[pend_i1] = pend_summary;            // one word per 4 KiB
        }

        const uint64_t next = wt + wstride;
        PartDev npd = pd;
        uint64_t next_span = 0;
        const bool more = (int64_t)(next - nwt) < 0; // (the sign of a scalar difference: no 64-bit constant in vector registers)
        if (more)
        {
            npd = parts[tile_part[next >> 2]];
            next_span = ((next >> 2) - npd.tile_base) * (uint64_t)TILE + (next & 3u) * (uint64_t)WTILE;
            dma.issue(npd, next_span);
        }

        pend_m = prefix_legal(prefix_tile<MODE>(win, hb, pc, dv, lane, halo), span + (uint64_t)lane * RUN, pd.size);
        pend_summary = __builtin_amdgcn_ballot_w64(pend_m != 0ull);
        pend_i0 = pd.bm0_base + (span >> 6);
        pend_i1 = pd.bm1_base + (span >> 12);
        pend = true;

        if (!more)
            break;
        wt = next;
        pd = npd;
        span = next_span;
    }
    if (pend_m != 0ull)
        run_words(bm0, pend_i0)[(uint32_t)lane] = pend_m;
    if (lane == 0)
        bm1[pend_i1] = pend_summary;
}

// ---------------------------------------------------------------------------------------------------
// K2: one wave per part
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t bcast64(uint64_t v, int src_lane)
{
    uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, src_lane);
    uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), src_lane);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void k_select_cuts(const PartDev* __restrict__ parts, uint32_t nparts,
                                                    const uint64_t* __restrict__ bm0, const uint64_t* __restrict__ bm1,
                                                    uint32_t min_chunk, uint32_t max_chunk, uint2* __restrict__ region,
                                                    uint32_t* __restrict__ part_count)
{
    const uint32_t p = blockIdx.x;
    if (p >= nparts)
        return;
    const int lane = threadIdx.x;
    const PartDev pd = parts[p];
    const uint64_t size = pd.size;
    const uint64_t* b0 = bm0 + pd.bm0_base;
    const uint64_t* b1 = bm1 + pd.bm1_base;
    uint2* out = region + pd.region_base;

    uint64_t s = 0;
    uint32_t n = 0;
    while (s < size)
    {
        const uint64_t left = size - s;
        uint64_t len;
        if (left <= min_chunk)
            len = left; // hpcdcchunker.c:257-264
        else
        {
            const uint64_t end = left > max_chunk ? max_chunk : left; // :284
            len = end;
            // a cut of length L needs candidate bit q = s+L-1, L in [min+1, end]
            const uint64_t qlo = s + min_chunk;
            const uint64_t qhi = s + end - 1;
            if (qlo <= qhi)
            {
                const uint64_t rlo = qlo >> 6, rhi = qhi >> 6; // 64-byte runs
                const uint64_t wlo = rlo >> 6, whi = rhi >> 6; // level-1 words
                bool found = false;
                for (uint64_t w0 = wlo; w0 <= whi && !found; w0 += 64)
                {
                    const uint64_t w = w0 + (uint64_t)lane;
                    uint64_t word = 0;
                    if (w <= whi)
                    {
                        word = b1[w];
                        if (w == wlo)
                            word &= ~0ull << (rlo & 63);
                        if (w == whi && (rhi & 63) != 63)
                            word &= (1ull << ((rhi & 63) + 1)) - 1ull;
                    }
                    for (;;)
                    {
                        const uint64_t any = __builtin_amdgcn_ballot_w64(word != 0ull);
                        if (any == 0ull)
                            break;
                        const int f = __builtin_ctzll(any);
                        const uint64_t fw = bcast64(word, f);
                        const int bit = __builtin_ctzll(fw);
                        const uint64_t r = ((w0 + (uint64_t)f) << 6) + (uint64_t)bit;
                        uint64_t m = b0[r]; // wave-uniform address
                        if (r == rlo)
                            m &= ~0ull << (qlo & 63);
                        if (r == rhi && (qhi & 63) != 63)
                            m &= (1ull << ((qhi & 63) + 1)) - 1ull;
                        if (m != 0ull)
                        {
                            const uint64_t q = (r << 6) + (uint64_t)__builtin_ctzll(m);
                            len = q - s + 1;
                            found = true;
                            break;
                        }
                        if (lane == f)
                            word &= word - 1ull; // drop that run, try the next flagged one
                    }
                }
            }
        }
        if (lane == 0)
            out[n] = make_uint2((uint32_t)s, (uint32_t)len);
        ++n;
        s += len;
    }
    if (lane == 0)
        part_count[p] = n;
}

// ---------------------------------------------------------------------------------------------------
// K1 + K2 in one, the WALKING scan: a wave owns a whole part and walks it chunk by chunk.  HASH: K3's leaf pass as well.
//
// k_select_cuts reads only the candidate bits q in [s + min, s + end - 1] of a chunk that starts at s, and a candidate at q depends on
// the bytes [q - 47, q] alone: the first min - 47 bytes of every chunk are hashed for nothing by a scan that does not know where the
// chunks start.  A wave that walks its part serially knows: it jumps to the 64 bytes in front of s + min, hashes 4 KiB wave-tiles
// (prefix_tile, the table, the DMA staging and the workgroup shape of k_buzhash_prefix_dma, unchanged) until the first legal
// candidate, emits the chunk -- region[] and part_count[] exactly as k_select_cuts writes them -- and jumps again.  H is a pure
// function of the 48 bytes before a position, so the de-rotated frame of prefix_tile is simply local to the tile and a tile may start
// at any multiple of 16 (the DMA's source alignment).  Parts are drawn by ticket; everything the walk carries (s, the tile, the chunk
// count) is wave-uniform.  GUESS: the next tile's DMA is issued before this tile is hashed, aimed at where the walk goes if this tile
// holds no cut (the next 4 KiB, or the jump target behind a chunk that ends at `end`); a cut makes the guess wrong, and the tile is
// issued again.  Without it a tile's DMA is issued when the walk knows where it goes (ablation build: the measured alternative).
// Needs many more parts than resident waves (the host decides: plan_walk_rule, lthip_ctx.hip).
// The walk is ONE loop: a part is drawn, a chunk that needs no scan is emitted, a tile is hashed, or (HASH) a round is run, one of them
// per trip.  So the round stands at one place in the code (it is three compressions long), and every emission is followed by the test
// for a round before the next one.
//
// HASH: the waves hash the chunks they cut.  The scan leaves a SIMD's issue slots about a quarter idle (LDS round trips of the table
// look-ups) and the leaf pass is pure vector issue, so waves that scan and waves that hash fill each other's holes when they share a
// SIMD.  Here they are the same waves: a wave that emits a chunk holds its (s, len) in scalars, so it appends it to a pending list of
// its own in LDS -- {byte offset in data, len, chaining-value slot of its first leaf} -- and whenever 64 leaves are pending it runs one
// round of b3_leaf (k_blake3_leaf.h: the body of k_blake3_leaves), a leaf per lane.  A lane finds its (chunk, leaf) by a wave scan over
// the pending chunks' leaf counts.  The list is the only hand-off (no lane reads region[] back), it carries across parts, so only a
// wave's last round is short, and a chunk of more than 64 leaves spans rounds.  Nothing waits for another wave.
// At most 63 leaves are pending in front of an emission, so the list never holds more than 64 chunks, and behind a round of 64 only
// (the rest of) the last chunk is left.  Rounds run between tiles, where the walk's state is scalar and the tile's registers are dead; a
// guessed tile may be on its way into the buffer meanwhile (the list has LDS of its own).  A tile with several cuts (min < 4 KiB) is
// left when the list fills up and hashed again behind the round.
// Chaining values go to the part's run of cv_runs (lthip_part_run_base), densely from its start in chunk order: leaf k of a chunk at
// slot + k.  Flags and counter are the leaf kernel's.  region[] and part_count[] are the same with and without HASH.
// ---------------------------------------------------------------------------------------------------
#ifdef LTHIP_ABLATIONS
__device__ unsigned long long g_walk_tiles; // wave-tiles hashed by the walking scans of this process (lthip_debug_walk_tiles)
#endif

template <int MODE, int WAVES, bool GUESS, bool HASH>
__device__ __forceinline__ void walk_body(const uint8_t* __restrict__ data, const PartDev* __restrict__ parts, uint32_t nparts, DivTest dv,
                                          uint32_t min_chunk, uint32_t max_chunk, uint2* __restrict__ region,
                                          uint32_t* __restrict__ part_count, uint32_t* __restrict__ ticket, uint32_t* __restrict__ cv_runs)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const WaveLds lds = wave_lds<WAVES>(smem, __builtin_amdgcn_readfirstlane(tid >> 6));
    uint32_t* const halo = lds.halo;
    [[maybe_unused]] uint4* const pend = lds.pend;
    prefix_table_init(smem, tid, 64 * WAVES);

    const TileDma dma(data, lds.buf, lane);
    const PrefixConsts pc = dma.consts<MODE>(dv);
    const int lane_base = lane * RUN;

    // the tile whose data starts at or below candidate q (>= 48) with the 64 bytes in front of it as the halo row
    auto jump = [](uint64_t q) __attribute__((always_inline)) { return q >= 64 ? ((q - 64) & ~(uint64_t)15) + 64 : (uint64_t)0; };

    bool inflight = false; // a guessed tile is on its way into the buffer
    uint64_t inflight_tb = 0;
#ifdef LTHIP_ABLATIONS
    uint32_t tiles = 0;
#endif
    // (HASH) the pending list: pn chunks with pl leaves still to hash, phead of them of chunk 0 hashed already; last_nl = leaves of the
    // newest chunk; slot = the chaining-value slot of the next chunk's first leaf
    [[maybe_unused]] uint32_t pn = 0, pl = 0, phead = 0, last_nl = 0, slot = 0;
    // the walk (all wave-uniform): a part in hand, a chunk of it that needs a scan over the candidates [qlo, qhi], the tile at tb
    bool have = false, scanning = false, drained = false;
    PartDev pd = {};
    uint32_t t = 0, n = 0, end = 0;
    uint64_t size = 0, s = 0, qlo = 0, qhi = 0, tb = 0;
    uint2* out = region;

    auto emit = [&](uint32_t len) __attribute__((always_inline))
    {
        if (lane == 0)
        {
            [[maybe_unused]] const uint64_t at = pd.off + s;
            out[n] = make_uint2((uint32_t)s, len);
            if constexpr (HASH)
                pend[pn] = make_uint4((uint32_t)at, (uint32_t)(at >> 32), len, slot);
        }
        if constexpr (HASH)
            last_nl = leaves_of(len);
        ++n;
        if constexpr (HASH)
        {
            ++pn;
            pl += last_nl;
            slot += last_nl;
        }
        s += len;
    };
    // the chunk at s < size: true = it needs a scan (end, qlo, qhi set), false = it is `len` bytes without one (hpcdcchunker.c:257-264, and min == end)
    auto classify = [&](uint32_t& len) __attribute__((always_inline)) -> bool
    {
        const uint64_t left = size - s;
        len = left <= min_chunk ? (uint32_t)left : left > max_chunk ? max_chunk : (uint32_t)left; // :284
        if (!(left > min_chunk && len > min_chunk))
            return false;
        end = len;
        qlo = s + min_chunk; // a cut of length L needs candidate bit q = s + L - 1, L in [min + 1, end]
        qhi = s + end - 1;
        return true;
    };

    for (;;)
    {
        if constexpr (HASH)
            if (pl >= 64u || (drained && pl != 0u))
            {
                // ---- one round: lane L hashes pending leaf L ----
                asm volatile("" ::: "memory"); // lane 0's list entries are in LDS in front of the lanes' reads (one wave: LDS is in order)
                __builtin_amdgcn_wave_barrier();
                const bool has = (uint32_t)lane < pn;
                const uint4 e = pend[has ? lane : 0];
                const uint32_t cnt = has ? leaves_of(e.z) - (lane == 0 ? phead : 0u) : 0u;
                uint32_t incl = cnt; // inclusive scan over the lanes
                incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xf, 0xf, false); // row_shr:1
                incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xf, 0xf, false); // row_shr:2
                incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xf, 0xf, false); // row_shr:4
                incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xf, 0xf, false); // row_shr:8
                incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xa, 0xf, false); // row_bcast:15
                incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xc, 0xf, false); // row_bcast:31
                const uint32_t excl = incl - cnt;
                if (!has)
                    incl = 0xFFFFFFFFu;
                const uint32_t take = pl < 64u ? pl : 64u;
                // chunk j of the list holds leaf L: j = the chunks whose leaves end at or below L (incl is ascending; L < take <= incl[pn - 1])
                uint32_t j = 0;
#pragma unroll
                for (uint32_t step = 32u; step; step >>= 1)
                    if ((uint32_t)__builtin_amdgcn_ds_bpermute((int)((j + step - 1u) * 4u), (int)incl) <= (uint32_t)lane)
                        j += step;
                const bool on = (uint32_t)lane < take;
                if (!on)
                    j = 0;
                const uint32_t k = (uint32_t)lane - (uint32_t)__builtin_amdgcn_ds_bpermute((int)(j * 4u), (int)excl) + (j == 0u ? phead : 0u);
                const uint4 c = pend[j];
                if (on)
                {
                    uint32_t cv[8];
                    b3_leaf(cv, data + (((uint64_t)c.y << 32) | c.x) + ((uint64_t)k << 10), c.z, k);
                    uint4* o = reinterpret_cast<uint4*>(cv_runs + (uint64_t)(c.w + k) * 8u);
                    o[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
                    o[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
                }
                pl -= take;
                if (pl != 0u) // (the rest of) the newest chunk
                {
                    const uint32_t li = pn - 1u;
                    const uint4 l = make_uint4(__builtin_amdgcn_readlane(e.x, li), __builtin_amdgcn_readlane(e.y, li),
                                               __builtin_amdgcn_readlane(e.z, li), __builtin_amdgcn_readlane(e.w, li));
                    if (lane == 0)
                        pend[0] = l;
                    phead = last_nl - pl;
                    pn = 1;
                }
                else
                    pn = 0, phead = 0;
                asm volatile("" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                continue;
            }
        if (drained)
            break;
        if (!have)
        {
            // Every lane takes part in the draw (lane 0 adds one, the others zero): no lane-dependent branch around the loop-carried
            // ticket (the compiler hazard)
            __builtin_amdgcn_wave_barrier();
            t = atomicAdd(ticket, lane == 0 ? 1u : 0u);
            t = __builtin_amdgcn_readfirstlane(t);
            if (t >= nparts)
            {
                drained = true;
                continue;
            }
            pd = parts[t];
            size = pd.size;
            out = region + pd.region_base;
            if constexpr (HASH)
                slot = (uint32_t)lthip_part_run_base(pd);
            s = 0;
            n = 0;
            have = true;
            scanning = false;
        }
        if (!scanning)
        {
            if (s >= size) // the part is done
            {
                if (inflight)
                {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // nothing may land in the buffer behind the next part's first tile
                    inflight = false;
                }
                if (lane == 0)
                    part_count[t] = n;
                have = false;
                continue;
            }
            uint32_t len;
            if (!classify(len))
            {
                emit(len);
                continue;
            }
            tb = jump(qlo); // part-relative start of the tile's data
            scanning = true;
        }

        // ---- one tile ----
        // whether the chunk's last legal candidate lies in the tile at tb.  tb <= qlo <= qhi < size < 2^32 whenever a tile is hashed
        // (tb = jump(qlo), or moved on by a tile because qhi lay behind it), so the distance is a 32-bit scalar
        auto ends_here = [&]() __attribute__((always_inline)) { return (uint32_t)(qhi - tb) < (uint32_t)WTILE; };
        if (!(inflight && inflight_tb == tb))
        {
            if (inflight)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the wrong guess has to land before the buffer is aimed at again
            dma.issue(pd, tb);
        }
        inflight = false;
        uint32_t win[16], hb;
        dma.take(win, hb, pc);
        if (GUESS)
        {
            uint64_t g = tb + (uint64_t)WTILE; // no cut in this tile: the chunk goes on ...
            bool aim = true;
            if (ends_here()) // ... or ends at `end`, and the walk jumps
            {
                const uint64_t s2 = s + end;
                aim = size - s2 > min_chunk && max_chunk > min_chunk;
                g = jump(s2 + min_chunk);
            }
            if (aim)
            {
                dma.issue(pd, g);
                inflight = true;
                inflight_tb = g;
            }
        }
        const uint64_t raw = prefix_tile<MODE>(win, hb, pc, dv, lane, halo); // bit k <=> candidate tb + lane_base + k
#ifdef LTHIP_ABLATIONS
        ++tiles;
#endif
        for (;;) // the chunks that end in this tile
        {
            // the legal bits of the run: [qlo, qhi] relative to the tile, then to the run (beyond the part: qhi < size)
            const int lo = (int)(qlo > tb ? qlo - tb : 0) - lane_base;
            const int hi = (int)(ends_here() ? (uint32_t)(qhi - tb) : (uint32_t)WTILE - 1u) - lane_base;
            uint64_t m = raw;
            if (lo > 0)
                m = lo > 63 ? 0ull : m & (~0ull << lo);
            if (hi < 63)
                m = hi < 0 ? 0ull : m & ((2ull << hi) - 1ull);
            const uint64_t any = __builtin_amdgcn_ballot_w64(m != 0ull);
            uint32_t len;
            if (any != 0ull)
            {
                const int f = __builtin_ctzll(any);
                const uint64_t q = tb + (uint64_t)(f * RUN + __builtin_ctzll(bcast64(m, f)));
                len = (uint32_t)(q - s) + 1u;
            }
            else if (ends_here())
                len = end; // no candidate up to the last legal one
            else
            {
                tb += (uint64_t)WTILE; // the chunk goes on in the next tile, whose halo row is this tile's last 64 bytes
                break;
            }
            emit(len);
            uint32_t plain;
            if (s >= size || !classify(plain)) // the part's end, or a chunk without a scan: the head of the loop deals with both
            {
                scanning = false;
                break;
            }
            // (tb < s <= qlo < size: the chunk before ended in this tile)
            if ((uint32_t)(qlo - tb) < (uint32_t)WTILE && (!HASH || pl < 64u))
                continue; // (min < 4 KiB) the next chunk's first candidate lies in this tile as well
            tb = jump(qlo); // (HASH, a full list: this very tile again, behind the round)
            break;
        }
    }
#ifdef LTHIP_ABLATIONS
    if (lane == 0 && tiles)
        atomicAdd(&g_walk_tiles, (unsigned long long)tiles);
#endif
}

template <int MODE, int WAVES, bool GUESS>
__global__ __launch_bounds__(64 * WAVES, 1) void k_buzhash_walk(const uint8_t* __restrict__ data, const PartDev* __restrict__ parts,
                                                                 uint32_t nparts, DivTest dv, uint32_t min_chunk, uint32_t max_chunk,
                                                                 uint2* __restrict__ region, uint32_t* __restrict__ part_count,
                                                                 uint32_t* __restrict__ ticket)
{
    walk_body<MODE, WAVES, GUESS, false>(data, parts, nparts, dv, min_chunk, max_chunk, region, part_count, ticket, nullptr);
}

template <int MODE, int WAVES, bool GUESS>
__global__ __launch_bounds__(64 * WAVES, 1) void k_buzhash_hash_walk(const uint8_t* __restrict__ data, const PartDev* __restrict__ parts,
                                                                      uint32_t nparts, DivTest dv, uint32_t min_chunk, uint32_t max_chunk,
                                                                      uint2* __restrict__ region, uint32_t* __restrict__ part_count,
                                                                      uint32_t* __restrict__ ticket, uint32_t* __restrict__ cv_runs)
{
    walk_body<MODE, WAVES, GUESS, true>(data, parts, nparts, dv, min_chunk, max_chunk, region, part_count, ticket, cv_runs);
}

// ---------------------------------------------------------------------------------------------------
// scans + compaction
// ---------------------------------------------------------------------------------------------------
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* total, uint32_t* sh /*>= 8*/)
{
    // wave scan (DPP-free, shuffles) + cross-wave combine
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
        uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o)
            x += y;
    }
    if (lane == 63)
        sh[wave] = x;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w)
    {
        uint32_t t = sh[w];
        if (w < wave)
            base += t;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return base + x - v;
}

// pass 1: per-block sums
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_sums(const uint32_t* __restrict__ in, uint64_t n,
                                                            const uint32_t* __restrict__ n_dev,
                                                            uint32_t* __restrict__ sums)
{
    __shared__ uint32_t sh[8];
    if (n_dev)
        n = *n_dev < n ? *n_dev : n;
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLOCK;
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
    {
        uint64_t idx = base + (uint64_t)i * SCAN_THREADS + threadIdx.x;
        if (idx < n)
            acc += in[idx];
    }
    uint32_t tot;
    block_exclusive_scan(acc, &tot, sh);
    if (threadIdx.x == 0)
        sums[blockIdx.x] = tot;
}

// pass 2: single block scans the block sums in place, writes grand total to sums[nblocks]
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_spine(uint32_t* __restrict__ sums, uint32_t nblocks)
{
    __shared__ uint32_t sh[8];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nblocks; b0 += SCAN_THREADS)
    {
        uint32_t i = b0 + threadIdx.x;
        uint32_t v = i < nblocks ? sums[i] : 0;
        uint32_t tot;
        uint32_t ex = block_exclusive_scan(v, &tot, sh);
        if (i < nblocks)
            sums[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0)
        sums[nblocks] = carry;
}

// pass 3: out[i] = exclusive prefix ; out[n] = total (out has n+1 entries)
__global__ __launch_bounds__(SCAN_THREADS) void k_scan_apply(const uint32_t* __restrict__ in, uint64_t n,
                                                             const uint32_t* __restrict__ n_dev,
                                                             const uint32_t* __restrict__ sums, uint32_t nblocks,
                                                             uint32_t* __restrict__ out)
{
    __shared__ uint32_t sh[8];
    if (n_dev)
        n = *n_dev < n ? *n_dev : n;
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_BLOCK + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
    {
        uint64_t idx = base + i;
        v[i] = idx < n ? in[idx] : 0;
        acc += v[i];
    }
    uint32_t tot;
    uint32_t ex = block_exclusive_scan(acc, &tot, sh) + sums[blockIdx.x];
#pragma unroll
    for (int i = 0; i < SCAN_ITEMS; ++i)
    {
        uint64_t idx = base + i;
        if (idx < n)
            out[idx] = ex;
        ex += v[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        out[n] = sums[nblocks];
}

// dense gather: one wave per part
__global__ __launch_bounds__(64) void k_compact_chunks(const PartDev* __restrict__ parts, uint32_t nparts,
                                                       const uint2* __restrict__ region,
                                                       const uint32_t* __restrict__ part_first,
                                                       uint64_t* __restrict__ chunk_offsets,
                                                       uint32_t* __restrict__ chunk_lens)
{
    const uint32_t p = blockIdx.x;
    if (p >= nparts)
        return;
    const PartDev pd = parts[p];
    const uint32_t first = part_first[p];
    const uint32_t n = part_first[p + 1] - first;
    const uint2* in = region + pd.region_base;
    for (uint32_t i = threadIdx.x; i < n; i += 64)
    {
        uint2 e = in[i];
        chunk_offsets[first + i] = pd.off + (uint64_t)e.x;
        chunk_lens[first + i] = e.y;
    }
}

// ---------------------------------------------------------------------------------------------------
// NextChunkFromBuffer (hpcdcchunker.c:452-523): one wave, every lane evaluates the hash of one candidate
// length directly.  For the first 47 lengths after `min` the reference's rolling window still holds bytes
// buf[0..48) (it is seeded from the FRONT of the buffer, :488-494), so
//   h(k) = rotl(h0,k) ^ XOR_{i=1..k} rotl( rotl(T[buf[i-1]],16) ^ T[buf[min+i-1]], k-i ),  h0 = XOR_i rotl(T[buf[i]],47-i)
// and from k = 48 on it is the ordinary 48-byte window hash.
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_chunk_from_buffer(const uint8_t* __restrict__ buf, uint32_t n, uint32_t min_chunk,
                                                          DivTest dv, uint64_t* __restrict__ out_len)
{
    const int lane = threadIdx.x;
    uint32_t h0 = 0;
    for (uint32_t i = 0; i < 48; ++i)
        h0 ^= rotl32(c_buztab[buf[i]], (47u - i) & 31u);
    uint32_t result = n;
    const uint32_t kmax = n - min_chunk; // candidate lengths min+1 .. n
    for (uint32_t k0 = 1; k0 <= kmax; k0 += 64)
    {
        const uint32_t k = k0 + (uint32_t)lane;
        bool hit = false;
        if (k <= kmax)
        {
            uint32_t h;
            if (k < 48)
            {
                h = rotl32(h0, k & 31u);
                for (uint32_t i = 1; i <= k; ++i)
                    h ^= rotl32(rotl32(c_buztab[buf[i - 1]], 16) ^ c_buztab[buf[min_chunk + i - 1]], (k - i) & 31u);
            }
            else
            {
                const uint32_t p = min_chunk + k; // window = the 48 bytes before p
                h = 0;
                for (uint32_t j = 0; j < 48; ++j)
                    h ^= rotl32(c_buztab[buf[p - 1 - j]], j & 31u);
            }
            hit = dv.pow2 ? (h & (dv.d - 1u)) == dv.d - 1u : rotr32(h * dv.inv + dv.addc, dv.k2) <= dv.qlim;
        }
        const uint64_t any = __builtin_amdgcn_ballot_w64(hit);
        if (any)
        {
            result = min_chunk + k0 + (uint32_t)__builtin_ctzll(any);
            break;
        }
    }
    if (lane == 0)
        *out_len = result;
}

} // namespace

int lthip_launch_from_buffer(lthip_ctx* ctx, const uint8_t* d_data, uint32_t n, uint32_t min_chunk, const DivTest& dv,
                             uint64_t* d_out)
{
    LaunchTimer t(ctx, LTHIP_K_OTHER);
    hipLaunchKernelGGL(k_chunk_from_buffer, dim3(1), dim3(64), 0, ctx->stream, d_data, n, min_chunk, dv, d_out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------
int lthip_launch_tile_table(lthip_ctx* ctx, lthip_plan* plan)
{
    if (plan->ntiles == 0)
        return 0;
    LaunchTimer t(ctx, LTHIP_K_OTHER);
    const uint32_t blocks = (uint32_t)div_up_u64(plan->ntiles, 256);
    hipLaunchKernelGGL(k_tile_table, dim3(blocks), dim3(256), 0, ctx->stream, plan->d_parts, plan->nparts,
                       plan->d_tile_part, plan->ntiles);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

#ifdef LTHIP_ABLATIONS
constexpr bool K1_HAS_REG_FLAVOUR = true;
#else
constexpr bool K1_HAS_REG_FLAVOUR = false;
#endif

template <int WAVES, bool DMA>
static int launch_buzhash_prefix(lthip_ctx* ctx, const lthip_plan* plan, const uint8_t* d_data, uint64_t* bm0, uint64_t* bm1)
{
    static_assert(DMA || K1_HAS_REG_FLAVOUR, "the register-staged flavour is compiled by the ablation build only");
    // (the register-staged flavour: padded rows in place of the linear buffer, ablations/k_buzhash_prefix_regs.inc)
    constexpr size_t lds = DMA ? lds_bytes(WAVES, false) : sizeof(uint32_t) * (TAB_DW + WAVES * (WROWS * ROW_DW + HALO_DW));
    static_assert(lds <= 160 * 1024, "LDS budget: one workgroup per CU");
#ifdef LTHIP_ABLATIONS
    auto k0 = DMA ? &k_buzhash_prefix_dma<0, WAVES> : &k_buzhash_prefix<0, WAVES>;
    auto k1 = DMA ? &k_buzhash_prefix_dma<1, WAVES> : &k_buzhash_prefix<1, WAVES>;
#else
    auto k0 = &k_buzhash_prefix_dma<0, WAVES>;
    auto k1 = &k_buzhash_prefix_dma<1, WAVES>;
#endif
    static std::atomic<bool> granted[64] = {};
    if (int err = lthip_grant_lds(ctx, granted, {reinterpret_cast<const void*>(k0), reinterpret_cast<const void*>(k1)}, lds))
        return err;
    uint32_t grid = lthip_cu_count(ctx->device);
    if ((uint64_t)grid * WAVES > plan->ntiles * 4u)
        grid = (uint32_t)div_up_u64(plan->ntiles * 4u, WAVES);
    LaunchTimer t(ctx, LTHIP_K_BUZHASH);
    hipLaunchKernelGGL(plan->div.pow2 ? k1 : k0, dim3(grid), dim3(64 * WAVES), lds, ctx->stream, d_data, plan->d_parts,
                       plan->d_tile_part, (uint32_t)plan->ntiles, plan->div, bm0, bm1);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

#ifdef LTHIP_ABLATIONS
// LTHIP_K1 (ablation build): "dma16" (the product's kernel) / "dma12" = the prefix-XOR kernel fed by LDS-DMA, 16 / 12 waves per CU;
// "prefix16" / "prefix12" = the same with register staging; "roll" = the rolling-window kernel of rounds 1-2
static int k1_flavour()
{
    // (read again after lthip_debug_reload_env: tools/ablations/k1_stress_tib.py runs two flavours against each other in one process)
    static std::atomic<int> f{-1};
    static std::atomic<uint32_t> seen{0};
    const uint32_t gen = g_lthip_env_gen;
    if (seen.load(std::memory_order_acquire) != gen)
    {
        const char* e = getenv("LTHIP_K1");
        f.store(!e ? 0 : !strcmp(e, "roll") ? 4 : !strcmp(e, "prefix12") ? 3 : !strcmp(e, "prefix16") ? 2 : !strcmp(e, "dma12") ? 1 : 0,
                std::memory_order_relaxed);
        seen.store(gen, std::memory_order_release);
    }
    return f.load(std::memory_order_relaxed);
}

static int launch_buzhash_roll(lthip_ctx* ctx, const lthip_plan* plan, const uint8_t* d_data, uint64_t* bm0, uint64_t* bm1)
{
    static_assert(sizeof(uint32_t) * (256 * TAB_REP + K1_WAVES * WROWS * ROW_DW) <= 160 * 1024, "LDS budget: one workgroup per CU");
    const size_t lds = sizeof(uint32_t) * (256 * TAB_REP + K1_WAVES * WROWS * ROW_DW);
    static std::atomic<bool> granted[64] = {};
    if (int err = lthip_grant_lds(ctx, granted, {reinterpret_cast<const void*>(&k_buzhash_candidates<0>), reinterpret_cast<const void*>(&k_buzhash_candidates<1>)}, lds))
        return err;
    // one persistent workgroup of 12 waves per CU (64 KiB table + 12 wave row buffers = 117 KiB of LDS)
    uint32_t grid = lthip_cu_count(ctx->device);
    if ((uint64_t)grid * K1_WAVES > plan->ntiles * 4u)
        grid = (uint32_t)div_up_u64(plan->ntiles * 4u, K1_WAVES);
    LaunchTimer t(ctx, LTHIP_K_BUZHASH);
    if (plan->div.pow2)
        hipLaunchKernelGGL(k_buzhash_candidates<1>, dim3(grid), dim3(K1_THREADS), lds, ctx->stream, d_data, plan->d_parts,
                           plan->d_tile_part, (uint32_t)plan->ntiles, plan->div, bm0, bm1);
    else
        hipLaunchKernelGGL(k_buzhash_candidates<0>, dim3(grid), dim3(K1_THREADS), lds, ctx->stream, d_data, plan->d_parts,
                           plan->d_tile_part, (uint32_t)plan->ntiles, plan->div, bm0, bm1);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}
#endif

int lthip_launch_buzhash(lthip_ctx* ctx, const lthip_plan* plan, const uint8_t* d_data, uint64_t* bm0, uint64_t* bm1)
{
    if (plan->ntiles == 0)
        return 0;
#ifdef LTHIP_ABLATIONS
    const int flavour = k1_flavour();
    if (flavour == 1)
        return launch_buzhash_prefix<12, true>(ctx, plan, d_data, bm0, bm1);
    if (flavour == 2)
        return launch_buzhash_prefix<16, false>(ctx, plan, d_data, bm0, bm1);
    if (flavour == 3)
        return launch_buzhash_prefix<12, false>(ctx, plan, d_data, bm0, bm1);
    if (flavour == 4)
        return launch_buzhash_roll(ctx, plan, d_data, bm0, bm1);
#endif
    return launch_buzhash_prefix<16, true>(ctx, plan, d_data, bm0, bm1);
}

// the device's compute units (256 where the runtime does not say)
uint32_t lthip_cu_count(int device)
{
    static std::atomic<uint32_t> cached[64] = {};
    if (device >= 0 && device < 64 && cached[device].load(std::memory_order_relaxed))
        return cached[device].load(std::memory_order_relaxed);
    int ncu = 256;
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
    const uint32_t n = (uint32_t)(ncu > 0 ? ncu : 256);
    if (device >= 0 && device < 64)
        cached[device].store(n, std::memory_order_relaxed);
    return n;
}

#ifndef K1_WALK_GUESS
#define K1_WALK_GUESS 1 // 1: the next tile's DMA in flight while this one is hashed, aimed again behind a cut; 0: decide first, then issue.
                        // Measured on the headline tree, alternating (profiles/walk_scan_sweep.txt): 891-893 against 895-896 GB/s, K1 alone
                        // 16.3 against 15.9 ms -- the plain form is 0.3-0.5 % ahead, inside the box's +-1 %.  The guess is the form the
                        // whole test file ran on; the other is LTHIP_K1_WALK_GUESS=0 in the ablation build.
#endif

template <int MODE, int WAVES, bool GUESS, bool HASH>
static constexpr auto walk_kernel()
{
    if constexpr (HASH)
        return &k_buzhash_hash_walk<MODE, WAVES, GUESS>;
    else
        return &k_buzhash_walk<MODE, WAVES, GUESS>;
}

// HASH: the scan that hashes the chunks it cuts (cv_runs), with the waves' pending lists behind the tile buffers
template <bool GUESS, bool HASH>
static int launch_buzhash_walk(lthip_ctx* ctx, const lthip_plan* plan, const uint8_t* d_data, uint2* region, uint32_t* part_count,
                               uint32_t* cv_runs)
{
    constexpr int WAVES = 16;
    constexpr size_t lds = lds_bytes(WAVES, HASH);
    static_assert(lds <= 160 * 1024 && (sizeof(uint32_t) * lds_pend_dw(WAVES)) % 16 == 0,
                  "LDS budget: one workgroup per CU; the lists are 16-byte aligned");
    const auto k0 = walk_kernel<0, WAVES, GUESS, HASH>(), k1 = walk_kernel<1, WAVES, GUESS, HASH>();
    static std::atomic<bool> granted[64] = {};
    int err = lthip_grant_lds(ctx, granted, {reinterpret_cast<const void*>(k0), reinterpret_cast<const void*>(k1)}, lds);
    if (err)
        return err;
    void* ticket;
    if ((err = lthip_scratch(ctx, S_WALK_TICKET, 64, &ticket)))
        return err;
    uint32_t grid = lthip_cu_count(ctx->device); // one 16-wave workgroup per CU (lthip_k1_resident_waves)
    if ((uint64_t)grid * WAVES > plan->nparts)
        grid = (uint32_t)div_up_u64(plan->nparts, WAVES);
    LaunchTimer t(ctx, LTHIP_K_BUZHASH);
    LTHIP_CHECK(ctx, hipMemsetAsync(ticket, 0, 4, ctx->stream));
    const auto k = plan->div.pow2 ? k1 : k0;
    if constexpr (HASH)
        hipLaunchKernelGGL(k, dim3(grid), dim3(64 * WAVES), lds, ctx->stream, d_data, plan->d_parts, plan->nparts, plan->div,
                           plan->min_chunk, plan->max_chunk, region, part_count, (uint32_t*)ticket, cv_runs);
    else
        hipLaunchKernelGGL(k, dim3(grid), dim3(64 * WAVES), lds, ctx->stream, d_data, plan->d_parts, plan->nparts, plan->div,
                           plan->min_chunk, plan->max_chunk, region, part_count, (uint32_t*)ticket);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

// the walking scan: candidate scan and cut selection of every part in one launch (region / part_count as lthip_launch_select leaves them)
int lthip_launch_buzhash_walk(lthip_ctx* ctx, const lthip_plan* plan, const uint8_t* d_data, uint2* region, uint32_t* part_count,
                              uint32_t* cv_runs)
{
    if (plan->nparts == 0)
        return 0;
#ifdef LTHIP_ABLATIONS
    LTHIP_ABLATION_ENV(env_guess, "LTHIP_K1_WALK_GUESS"); // 0 / 1: the other form of the prefetch
    if (env_guess.get() >= 0 && (env_guess.get() != 0) != (K1_WALK_GUESS != 0))
        return cv_runs ? launch_buzhash_walk<!K1_WALK_GUESS, true>(ctx, plan, d_data, region, part_count, cv_runs)
                       : launch_buzhash_walk<!K1_WALK_GUESS, false>(ctx, plan, d_data, region, part_count, nullptr);
#endif
    return cv_runs ? launch_buzhash_walk<K1_WALK_GUESS != 0, true>(ctx, plan, d_data, region, part_count, cv_runs)
                   : launch_buzhash_walk<K1_WALK_GUESS != 0, false>(ctx, plan, d_data, region, part_count, nullptr);
}

// (ablation build) wave-tiles the walking scans of this process have hashed since the last call; waits for the device
extern "C" int lthip_debug_walk_tiles(uint64_t* out_tiles)
{
#ifdef LTHIP_ABLATIONS
    if (!out_tiles)
        return EINVAL;
    unsigned long long v = 0, zero = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_walk_tiles), sizeof v) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(g_walk_tiles), &zero, sizeof zero) != hipSuccess)
        return EIO;
    *out_tiles = v;
    return 0;
#else
    (void)out_tiles;
    return ENOTSUP;
#endif
}

int lthip_launch_select(lthip_ctx* ctx, const lthip_plan* plan, const uint64_t* bm0, const uint64_t* bm1, uint2* region,
                        uint32_t* part_count)
{
    LaunchTimer t(ctx, LTHIP_K_SELECT);
    hipLaunchKernelGGL(k_select_cuts, dim3(plan->nparts), dim3(64), 0, ctx->stream, plan->d_parts, plan->nparts, bm0, bm1,
                       plan->min_chunk, plan->max_chunk, region, part_count);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

// d_out[i] = sum of d_in[0..i) for i in [0, n] where n = min(n_bound, *d_n) (d_n may be null); d_out holds n+1 entries
int lthip_exclusive_scan_u32(lthip_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, uint64_t n_bound,
                             const uint32_t* d_n, int kid)
{
    const uint64_t nblocks64 = n_bound ? div_up_u64(n_bound, SCAN_BLOCK) : 1;
    if (nblocks64 > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "scan", "too many elements");
    const uint32_t nblocks = (uint32_t)nblocks64;
    void* tmp;
    int err = lthip_scratch(ctx, S_SCAN_TMP, ((size_t)nblocks + 1) * 4, &tmp);
    if (err)
        return err;
    uint32_t* sums = (uint32_t*)tmp;
    LaunchTimer t(ctx, kid);
    hipLaunchKernelGGL(k_scan_sums, dim3(nblocks), dim3(SCAN_THREADS), 0, ctx->stream, d_in, n_bound, d_n, sums);
    hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(SCAN_THREADS), 0, ctx->stream, sums, nblocks);
    hipLaunchKernelGGL(k_scan_apply, dim3(nblocks), dim3(SCAN_THREADS), 0, ctx->stream, d_in, n_bound, d_n, sums, nblocks,
                       d_out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

int lthip_launch_compact(lthip_ctx* ctx, const lthip_plan* plan, const uint2* region, const uint32_t* part_count,
                         uint32_t* d_part_first, uint64_t* d_chunk_offsets, uint32_t* d_chunk_lens)
{
    int err = lthip_exclusive_scan_u32(ctx, part_count, d_part_first, plan->nparts, nullptr, LTHIP_K_COMPACT);
    if (err || plan->nparts == 0)
        return err;
    LaunchTimer t(ctx, LTHIP_K_COMPACT);
    hipLaunchKernelGGL(k_compact_chunks, dim3(plan->nparts), dim3(64), 0, ctx->stream, plan->d_parts, plan->nparts, region,
                       (const uint32_t*)d_part_first, d_chunk_offsets, d_chunk_lens);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}
