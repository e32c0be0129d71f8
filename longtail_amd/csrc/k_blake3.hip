// k_blake3.hip -- BLAKE3-64 chunk hashing on gfx950.
//
// Reference behaviour: Blake3Hash_HashBuffer (lib/blake3/longtail_blake3.c:81-102) = unkeyed BLAKE3, first 8
// output bytes as a little-endian u64; arithmetic per lib/blake3/ext/blake3_portable.c:8-98 (compression
// function), blake3_impl.h:85-97 (IV, message schedule), blake3.c:118-166, 216-249, 576-618 (leaf/"chunk"
// state machine, left-heavy tree, ROOT finalisation).
//
// MI355X formulation: pure 32-bit integer ALU work (no MFMA):
//   leaf kernel   one thread per 1 KiB leaf of every range: 16 state + 16 message words live in VGPRs, the 7
//                 rounds are fully unrolled with the message schedule folded into register names; ranges start
//                 at arbitrary byte offsets, so message words are rebuilt from 4-byte aligned dwords with one
//                 v_alignbit each.  Leaf -> range mapping is a binary search over the exclusive scan of leaf
//                 counts (no per-leaf descriptor traffic).
//   parent kernel left-heavy reduction of each range's chaining values (level by level, stride doubling ==
//                 blake3's compress_parents_parallel with the odd node carried up), ROOT on the last merge;
//                 writes output words 0,1 as the u64 digest.  Small trees (<= 256 leaves): a workgroup per
//                 window of 2048 leaf slots, the two lowest levels in registers (a thread per aligned block
//                 of four leaves, read straight from global memory), the others lane-dense in LDS from a
//                 merge list that each level filters for the next.  Big trees: one launch per level, in place.
#include "lthip_internal.h"

#include <stdlib.h>

namespace
{

#include "k_blake3_leaf.h" // the compression function and the hashing of one leaf

// ---------------------------------------------------------------------------------------------------
// leaf counts
// ---------------------------------------------------------------------------------------------------

__global__ void k_leaf_counts(const uint32_t* __restrict__ lens, uint64_t bound, const uint32_t* __restrict__ n_dev,
                              uint32_t* __restrict__ counts)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t n = n_dev ? (*n_dev < bound ? *n_dev : bound) : bound;
    if (i < n)
        counts[i] = leaves_of(lens[i]);
}

// ---------------------------------------------------------------------------------------------------
// small trees: windows and blocks (parents kernel; the leaf kernel notes each window's first range)
// ---------------------------------------------------------------------------------------------------
// The small-tree parents kernel (k_blake3_parents_window, below) and the one line of the leaf kernel that notes a window's first
// range share these.  A range of n leaves is cut into blocks of B = 2^J leaf slots, block b holding leaves [b B, min(b B + B, n)):
// the node over a block is a node of the range's left-heavy tree (the stride doubling of the level reducers, restricted to the
// block), so a block is merged in one thread's registers and only its node goes on to the levels in LDS.
// The functions between the two marks are all the shape arithmetic of that kernel; a host compiler takes them as they are
// (tests/test_blake3_parents_shapes.py cuts them out and walks them for every n).
// [b3-parents-shapes
constexpr uint32_t b3s_blocks(uint32_t n, uint32_t B) { return (n + B - 1u) / B; } // blocks of a range of n leaves
constexpr uint32_t b3s_block_leaves(uint32_t n, uint32_t b, uint32_t B) { return n - b * B < B ? n - b * B : B; } // leaves of block b
// register stage, a block of m leaves: for st = 1, 2, .. < B, for k = 0, 2 st, .. < B in that order, leaf k takes leaf k + st
constexpr bool b3s_reg_merge(uint32_t m, uint32_t k, uint32_t st) { return k + st < m; }
// ROOT is on the merge at stride st (in leaves) whose left child is leaf K of a range of n leaves
constexpr bool b3s_root(uint32_t n, uint32_t K, uint32_t st) { return K == 0u && 2u * st >= n; }
// a range of more than one block sends every block's node to LDS; the node of a one-block range is its digest
constexpr bool b3s_to_lds(uint32_t n, uint32_t B) { return b3s_blocks(n, B) > 1u; }
// LDS levels, st = 1, 2, .. in BLOCKS: block k of a range of nb blocks takes block k + st.  The list of level 2 st is the part of
// level st's list for which this holds again (a left child at 2 st was one at st)
constexpr bool b3s_lds_merge(uint32_t nb, uint32_t k, uint32_t st) { return (k & (2u * st - 1u)) == 0u && k + st < nb; }
constexpr bool b3s_lds_root(uint32_t nb, uint32_t st) { return 2u * st >= nb; } // (then k = 0: it is b3s_root in blocks)
// most nodes in LDS for S leaf slots of ranges: ceil(n / B) <= 2 n / (B + 1) for every n > B, with equality at n = B + 1
constexpr uint32_t b3s_max_nodes(uint32_t S, uint32_t B) { return 2u * S / (B + 1u); }
// LDS bytes of a window of S leaf slots: a range has three 16-bit table entries and 32 bytes per node, which is at most 6 bytes per
// slot for a range of one block (n >= 1) and (6 + 64) / (B + 1) for the others (n = B + 1 again); tables and nodes share one
// array, because the window with the most ranges (all of one leaf) has no node and the one with the most nodes has few ranges
constexpr uint32_t b3s_range_bytes(uint32_t n, uint32_t B) { return 6u + (b3s_to_lds(n, B) ? 32u * b3s_blocks(n, B) : 0u); }
constexpr uint32_t b3s_max_bytes(uint32_t S, uint32_t B) { return (6u * (B + 1u) > 70u ? 6u * (B + 1u) : 70u) * S / (B + 1u) + 6u + 16u; }
// b3-parents-shapes]

constexpr uint32_t PJ = 2;
constexpr uint32_t PB = 1u << PJ; // leaf slots of a block
constexpr int PW = 2048;          // parents kernel: window of leaf slots per workgroup (a power of two)
constexpr int PW_MAXN = 256;      // leaves of the largest range (small trees: <= 256 KiB)
constexpr int PW_THREADS = 512;   // threads of a parents workgroup (a multiple of 64)
constexpr int PW_WAVES = 8;       // waves per SIMD the kernel is compiled for: FOUR workgroups per CU (32 waves; 4 x 36 KiB of LDS)
// Measured on the 64 GiB tree (same box, builds side by side through LTHIP_LIB_PATH; the kernel before this one, every level in LDS
// with a window of 1024, 2.80 ms): J = 1 / 2 / 3 with windows of 1024 / 2048 / 2048 slots and 512 / 512 / 256 threads 2.20 / 1.85 /
// 1.91 ms (J = 3 needs 92 registers: five workgroups of four waves).  Workgroups per CU decide more than anything else: J = 2 with
// tables and nodes in arrays of their own (45 KiB, three per CU) 2.03; 576 / 640 threads (one trip through the register stage, but
// 9 / 10 waves a workgroup) 2.57 / 2.43; J = 3 with 320 / 384 threads 2.61 / 3.07, with a window of 4096 and two per CU 2.32; J = 2
// with 1024 slots and 256 threads 2.13.  (profiles/b3_parents_ab.txt)
constexpr uint32_t PW_NODES = b3s_max_nodes(PW + PW_MAXN - 1, PB) + 1u;          // a window's slots: PW - 1 + 256 at the most
constexpr uint32_t PW_MEM16 = (b3s_max_bytes(PW + PW_MAXN - 1, PB) + 15u) / 16u; // uint4s of tables and nodes
constexpr uint32_t PW_LEVELS = 8u - PJ;                                          // 2^PW_LEVELS blocks in the largest range
static_assert(PW <= 4096 && (PW & (PW - 1)) == 0 && PW_THREADS % 64 == 0 && PW_MAXN >> PJ <= 255, "window tables are 16 bits, list entries 16 + 8 + 8");

// ---------------------------------------------------------------------------------------------------
// leaves
// ---------------------------------------------------------------------------------------------------

// PIPE: the message dwords of block b + 1 are loaded while block b is compressed (two register sets that swap roles by name, the
// loop unrolled by two).  A lane's loads are 64-line gathers, one 16-byte piece per lane and the lanes 1 KiB apart; without the
// second set every block waits for all of its own in front of its compression and only the SIMD's other waves cover them.  The
// addresses read are the same in both forms: a block's 16 dwords, the dword behind an interior block (block b + 1's first, which
// the next trip reads anyway), and of the last block the dwords that hold a byte of the leaf.  !PIPE is the earlier loop, kept in
// the ablation build (LTHIP_B3_PREFETCH=0).
// Eight waves per SIMD are part of the launch bounds: they are what the kernel runs at (512 registers / 8 = 64 a wave), and without
// the bound the allocator spreads the same values over 69 registers (tests/test_k3_leaf_budget.py).
template <bool PIPE>
__global__ __launch_bounds__(256, 8) void k_blake3_leaves(const uint8_t* __restrict__ data,
                                                       const uint64_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ lens,
                                                       const uint32_t* __restrict__ leaf_prefix, // [count+1]
                                                       uint64_t count_bound, const uint32_t* __restrict__ n_dev,
                                                       uint32_t* __restrict__ cvs, uint32_t* __restrict__ win_first)
{
    const uint32_t count = (uint32_t)(n_dev ? (*n_dev < count_bound ? *n_dev : count_bound) : count_bound);
    const uint32_t total = leaf_prefix[count];
    const uint64_t g64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g64 >= total)
        return;
    const uint32_t g = (uint32_t)g64;
    // range c with leaf_prefix[c] <= g < leaf_prefix[c+1]
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (leaf_prefix[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t c = lo;
    const uint32_t first = leaf_prefix[c];
    const uint32_t k = g - first; // leaf index inside the range == BLAKE3 chunk counter
    if (win_first && (g & (uint32_t)(PW - 1)) == 0u)
        win_first[g / (uint32_t)PW] = k == 0u ? c : c + 1u; // first range that starts at or after this window (parents kernel)
    const uint32_t rlen = lens[c];
    const uint32_t nleaf = leaves_of(rlen);
    const uint32_t llen = rlen - (k << 10) < 1024u ? rlen - (k << 10) : 1024u; // 0 only for the empty range
    const uint8_t* p = data + offsets[c] + ((uint64_t)k << 10);
    const uint32_t root = nleaf == 1u ? (uint32_t)F_ROOT : 0u;

    const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
    const uint32_t sh = mis * 8u;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p - mis); // 4-byte aligned

    uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
    const uint32_t nblocks = llen ? (llen + 63u) >> 6 : 1u;

    if constexpr (PIPE)
    {
#include "k_blake3_leaf_body.inc" // (the text of b3_leaf, k_blake3_leaf.h, which the walking scan that hashes calls)
    }
    else
    {
        // interior blocks: the 64 bytes (and the spill-over dword when misaligned) are inside the leaf
        for (uint32_t b = 0; b + 1 < nblocks; ++b)
        {
            const uint32_t* src = q + b * 16u;
            uint32_t w[17];
            const u32x4_a4 v0 = *reinterpret_cast<const u32x4_a4*>(src);
            const u32x4_a4 v1 = *reinterpret_cast<const u32x4_a4*>(src + 4);
            const u32x4_a4 v2 = *reinterpret_cast<const u32x4_a4*>(src + 8);
            const u32x4_a4 v3 = *reinterpret_cast<const u32x4_a4*>(src + 12);
            w[0] = v0.x; w[1] = v0.y; w[2] = v0.z; w[3] = v0.w;
            w[4] = v1.x; w[5] = v1.y; w[6] = v1.z; w[7] = v1.w;
            w[8] = v2.x; w[9] = v2.y; w[10] = v2.z; w[11] = v2.w;
            w[12] = v3.x; w[13] = v3.y; w[14] = v3.z; w[15] = v3.w;
            w[16] = mis ? src[16] : 0u;
            uint32_t m[16];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                m[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
            b3_compress(cv, m, k, 64u, b == 0 ? (uint32_t)F_CHUNK_START : 0u);
        }
        // last block: 0..64 bytes, touch only dwords that hold at least one byte of the leaf
        const uint32_t b = nblocks - 1u;
        const uint32_t bl = llen - b * 64u;
        uint32_t w[17];
        b3_load_last(w, q + b * 16u, bl ? (mis + bl + 3u) >> 2 : 0u); // dwords that intersect [p, p+bl)
        b3_last_block(cv, w, sh, k, bl, (uint32_t)F_CHUNK_END | root | (b == 0 ? (uint32_t)F_CHUNK_START : 0u));
    }
    uint4* out = reinterpret_cast<uint4*>(cvs + (uint64_t)g * 8u);
    out[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    out[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
}

// ---------------------------------------------------------------------------------------------------
// parents
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void b3_parent(uint32_t* __restrict__ left, const uint32_t* __restrict__ right, uint32_t flags)
{
    uint32_t m[16];
    const uint4 a0 = reinterpret_cast<const uint4*>(left)[0], a1 = reinterpret_cast<const uint4*>(left)[1];
    const uint4 b0 = reinterpret_cast<const uint4*>(right)[0], b1 = reinterpret_cast<const uint4*>(right)[1];
    m[0] = a0.x; m[1] = a0.y; m[2] = a0.z; m[3] = a0.w; m[4] = a1.x; m[5] = a1.y; m[6] = a1.z; m[7] = a1.w;
    m[8] = b0.x; m[9] = b0.y; m[10] = b0.z; m[11] = b0.w; m[12] = b1.x; m[13] = b1.y; m[14] = b1.z; m[15] = b1.w;
    uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
    b3_compress(cv, m, 0u, 64u, flags);
    reinterpret_cast<uint4*>(left)[0] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    reinterpret_cast<uint4*>(left)[1] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
}

#ifdef LTHIP_ABLATIONS
#include "ablations/k_blake3_parents_small.inc"
#endif

// ONE small input (<= 64 KiB) in ONE launch, read where it lies -- pinned host memory, over the bus -- and answered into pinned host
// memory: the plugin layer's HashBuffer of a path string, a chunk-hash array or a block's hash array (src/longtail.c:1272, 2522,
// 3757), which used to cost two uploads, seven launches (counts, scan, leaves, parents) and a download per call.  Lane l hashes leaf
// l byte by byte (speed is irrelevant here: the call is a bus round trip), lane 0 reduces the tree.
constexpr uint32_t B3_ONE_PITCH = 1024u + 4u; // LDS bytes per staged leaf: lanes read their leaves a dword at a time, 257 dwords apart
__global__ __launch_bounds__(64) void k_blake3_one(const uint8_t* __restrict__ in, uint32_t len, uint64_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_one[]; // [8 x 64 chaining values][leaves x B3_ONE_PITCH bytes of input]
    uint32_t* s_cv = s_one;
    uint32_t* s_in = s_one + 64 * 8;
    const uint32_t lane = threadIdx.x;
    const uint32_t nleaf = leaves_of(len);
    // The input is the caller's PINNED HOST block as a rule (plugin_hash.c): a lane that reads its 1 KiB leaf where it lies pays a
    // trip over the link per load, sixteen dependent rounds of them (byte loads: 115 us per 1 KiB call, 16-byte loads: 47).  So the wave
    // first brings the whole input into LDS with coalesced 16-byte loads that are all in flight together, then every lane hashes its
    // leaf from there (tools/hash_latency.py: 8 KiB 130 -> 31 us per HashBuffer call; 17 of them are the launch and the wait).
    {
        const uint32_t nvec = (((uintptr_t)in & 15u) == 0u) ? len >> 4 : 0u;
        const uint4* in4 = reinterpret_cast<const uint4*>(in);
        for (uint32_t v0 = 0; v0 < nvec; v0 += 64u * 8u)
        {
            uint4 q[8];
#pragma unroll
            for (int u = 0; u < 8; ++u)
            {
                const uint32_t v = v0 + (uint32_t)u * 64u + lane;
                q[u] = v < nvec ? in4[v] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
            {
                const uint32_t v = v0 + (uint32_t)u * 64u + lane;
                if (v < nvec)
                {
                    uint32_t* d = s_in + (v >> 6) * (B3_ONE_PITCH / 4u) + (v & 63u) * 4u; // (64 vectors per leaf)
                    d[0] = q[u].x;
                    d[1] = q[u].y;
                    d[2] = q[u].z;
                    d[3] = q[u].w;
                }
            }
        }
        for (uint32_t j = (nvec << 4) + lane; j < len; j += 64u) // the tail (or everything, from an unaligned address): bytes
            reinterpret_cast<uint8_t*>(s_in)[(j >> 10) * B3_ONE_PITCH + (j & 1023u)] = in[j];
    }
    __syncthreads();
    if (lane < nleaf)
    {
        const uint32_t llen = len - (lane << 10) < 1024u ? len - (lane << 10) : 1024u;
        const uint32_t* pw = s_in + lane * (B3_ONE_PITCH / 4u);
        const uint8_t* p = reinterpret_cast<const uint8_t*>(pw);
        const uint32_t nblocks = llen ? (llen + 63u) >> 6 : 1u;
        uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
        for (uint32_t b = 0; b < nblocks; ++b)
        {
            const uint32_t bl = llen - b * 64u < 64u ? llen - b * 64u : 64u;
            uint32_t m[16];
            if (bl == 64u)
            {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    m[i] = pw[b * 16u + (uint32_t)i];
            }
            else
            {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    m[i] = 0u;
                for (uint32_t j = 0; j < bl; ++j)
                    m[j >> 2] |= (uint32_t)p[b * 64u + j] << (8u * (j & 3u));
            }
            uint32_t fl = b == 0 ? (uint32_t)F_CHUNK_START : 0u;
            if (b + 1 == nblocks)
                fl |= (uint32_t)F_CHUNK_END | (nleaf == 1u ? (uint32_t)F_ROOT : 0u);
            b3_compress(cv, m, lane, bl, fl);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            s_cv[lane * 8 + i] = cv[i];
    }
    __syncthreads();
    // the tree, level by level: the merges of a level are independent (left-heavy tree == in-place stride doubling with the odd node
    // carried), lane j takes the j-th of them (64 leaves: six rounds instead of 63 merges on one lane)
    for (uint32_t stride = 1; stride < nleaf; stride <<= 1)
    {
        const uint32_t last = (stride << 1) >= nleaf;
        const uint32_t k = lane * (stride << 1);
        if (k + stride < nleaf)
            b3_parent(s_cv + k * 8u, s_cv + (k + stride) * 8u, (uint32_t)F_PARENT | (last ? (uint32_t)F_ROOT : 0u));
        __syncthreads();
    }
    if (lane == 0)
        *out = (uint64_t)s_cv[0] | ((uint64_t)s_cv[1] << 32);
}

// ---------------------------------------------------------------------------------------------------
// Streaming (Blake3Hash_BeginContext / _Hash / _EndContext, lib/blake3/longtail_blake3.c:24-79; ext/blake3.c:462-618).
// The reference keeps O(1) state: a partial 1 KiB chunk and a stack of subtree chaining values (one per set bit of the chunk
// count).  Same here, with the stack in device memory and the unit of work a BATCH of 1024 full leaves (1 MiB):
//   k_blake3_stream_batch  leaves leaf0 .. leaf0 + 1023 of the stream -> their complete subtree's chaining value (1024 threads, ten
//                          merge levels in LDS) -> pushed onto the stack, followed by `merges` = trailing-zeros(batch count) parent
//                          compressions (equal-sized neighbours merge: blake3.c:add_chunk_chaining_value restated per batch)
//   k_blake3_stream_final  the rest of the stream (0 .. 1 MiB, never empty unless the whole stream is): its leaves in parallel, then
//                          one thread pushes them the same way and folds the stack from the top, ROOT on the last compression
//                          (blake3.c:576-618); the empty stream is the one empty ROOT leaf.
// A batch is only hashed once a byte beyond it has arrived (the host holds it back), so the final kernel always has the last leaf.
// ---------------------------------------------------------------------------------------------------
constexpr int B3S_LEAVES = 1024;

__global__ __launch_bounds__(B3S_LEAVES) void k_blake3_stream_batch(const uint8_t* __restrict__ data, uint32_t leaf0,
                                                                      uint32_t* __restrict__ stack, uint32_t depth_in, uint32_t merges)
{
    __shared__ uint32_t s_cv[B3S_LEAVES * 8];
    const uint32_t t = threadIdx.x;
    {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(data) + (size_t)t * 256u; // 16-byte aligned device buffer
        uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
        for (uint32_t b = 0; b < 16u; ++b)
        {
            uint32_t m[16];
            const uint4* q = reinterpret_cast<const uint4*>(p + b * 16u);
            const uint4 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
            m[0] = v0.x; m[1] = v0.y; m[2] = v0.z; m[3] = v0.w; m[4] = v1.x; m[5] = v1.y; m[6] = v1.z; m[7] = v1.w;
            m[8] = v2.x; m[9] = v2.y; m[10] = v2.z; m[11] = v2.w; m[12] = v3.x; m[13] = v3.y; m[14] = v3.z; m[15] = v3.w;
            b3_compress(cv, m, leaf0 + t, 64u, (b == 0 ? (uint32_t)F_CHUNK_START : 0u) | (b == 15u ? (uint32_t)F_CHUNK_END : 0u));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            s_cv[t * 8 + i] = cv[i];
    }
    __syncthreads();
    for (uint32_t stride = 1; stride < (uint32_t)B3S_LEAVES; stride <<= 1)
    {
        if ((t & (2u * stride - 1u)) == 0u)
            b3_parent(s_cv + t * 8u, s_cv + (t + stride) * 8u, (uint32_t)F_PARENT);
        __syncthreads();
    }
    if (t == 0)
    {
        uint32_t depth = depth_in;
        for (int i = 0; i < 8; ++i)
            stack[depth * 8u + i] = s_cv[i];
        ++depth;
        for (uint32_t m = 0; m < merges; ++m)
        {
            b3_parent(stack + (depth - 2u) * 8u, stack + (depth - 1u) * 8u, (uint32_t)F_PARENT);
            --depth;
        }
    }
}

__global__ __launch_bounds__(B3S_LEAVES) void k_blake3_stream_final(const uint8_t* __restrict__ tail, uint32_t tail_len, uint32_t leaf0,
                                                                      const uint32_t* __restrict__ stack, uint32_t depth_in,
                                                                      uint64_t* __restrict__ out)
{
    __shared__ uint32_t s_cv[B3S_LEAVES * 8];
    __shared__ uint32_t s_stack[64 * 8];
    const uint32_t t = threadIdx.x;
    const uint32_t nleaf = tail_len ? (tail_len + 1023u) >> 10 : (leaf0 == 0u ? 1u : 0u);
    const bool single = leaf0 == 0u && nleaf == 1u; // the whole stream is one leaf: it carries ROOT itself
    if (t < nleaf)
    {
        const uint32_t llen = tail_len - (t << 10) < 1024u ? tail_len - (t << 10) : 1024u;
        const uint8_t* p = tail + ((size_t)t << 10);
        const uint32_t nblocks = llen ? (llen + 63u) >> 6 : 1u;
        uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
        for (uint32_t b = 0; b < nblocks; ++b)
        {
            const uint32_t bl = llen - b * 64u < 64u ? llen - b * 64u : 64u;
            uint32_t m[16];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                m[i] = 0u;
            for (uint32_t j = 0; j < bl; ++j)
                m[j >> 2] |= (uint32_t)p[b * 64u + j] << (8u * (j & 3u));
            uint32_t fl = b == 0 ? (uint32_t)F_CHUNK_START : 0u;
            if (b + 1 == nblocks)
                fl |= (uint32_t)F_CHUNK_END | (single ? (uint32_t)F_ROOT : 0u);
            b3_compress(cv, m, leaf0 + t, bl, fl);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            s_cv[t * 8 + i] = cv[i];
    }
    for (uint32_t i = t; i < depth_in * 8u; i += (uint32_t)B3S_LEAVES)
        s_stack[i] = stack[i];
    __syncthreads();
    if (t != 0)
        return;
    if (single)
    {
        *out = (uint64_t)s_cv[0] | ((uint64_t)s_cv[1] << 32);
        return;
    }
    // every leaf but the last is pushed and merged eagerly: after leaf number g (0-based) the stack holds one subtree per set bit of
    // g + 1.  The stack counts BATCHES below the tail (leaf0 is a multiple of 1024, so its entries are the set bits of leaf0 >> 10
    // and sit below anything the tail pushes).
    uint32_t depth = depth_in;
    for (uint32_t j = 0; j + 1 < nleaf; ++j)
    {
        for (int i = 0; i < 8; ++i)
            s_stack[depth * 8u + i] = s_cv[j * 8u + i];
        ++depth;
        uint32_t cnt = leaf0 + j + 1u; // chunks so far
        while ((cnt & 1u) == 0u)      // equal-sized neighbours merge
        {
            b3_parent(s_stack + (depth - 2u) * 8u, s_stack + (depth - 1u) * 8u, (uint32_t)F_PARENT);
            --depth;
            cnt >>= 1;
        }
    }
    // the last leaf's value, folded with the stack from the top; ROOT on the final compression
    uint32_t* cur = s_cv + (nleaf - 1u) * 8u;
    while (depth > 0u)
    {
        uint32_t* left = s_stack + (depth - 1u) * 8u;
        b3_parent(left, cur, (uint32_t)F_PARENT | (depth == 1u ? (uint32_t)F_ROOT : 0u));
        cur = left;
        --depth;
    }
    *out = (uint64_t)cur[0] | ((uint64_t)cur[1] << 32);
}

// left <- parent(left, right), both in registers
__device__ __forceinline__ void b3_merge_regs(uint32_t (&left)[8], const uint32_t (&right)[8], uint32_t flags)
{
    const uint32_t m[16] = {left[0], left[1], left[2], left[3], left[4], left[5], left[6], left[7],
                            right[0], right[1], right[2], right[3], right[4], right[5], right[6], right[7]};
    uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
    b3_compress(cv, m, 0u, 64u, flags);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        left[i] = cv[i];
}

// the lanes of a wave with `is` put their entry on a list in LDS (all lanes of the wave call it together)
__device__ __forceinline__ void pw_append(bool is, uint32_t entry, uint32_t* list, uint32_t* cnt, int lane)
{
    const uint64_t mask = __builtin_amdgcn_ballot_w64(is);
    if (mask == 0)
        return;
    uint32_t base = 0;
    if (lane == 0)
        base = atomicAdd(cnt, (uint32_t)__builtin_popcountll(mask));
    base = __builtin_amdgcn_readfirstlane(base);
    if (is)
        list[base + (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = entry;
}

// small trees: a workgroup owns the ranges whose first leaf slot lies in its window of PW slots (at most PW - 1 + 256 slots, at
// most PW ranges) and reduces ALL of them, in two stages (shapes: b3s_* above).
//   tables    one scan over the window's ranges gives each its first leaf slot, first block and first node, 16 bits each
//   registers thread t takes the window's t-th block (a search of the block table finds its range), loads the block's chaining
//             values from global memory -- 32 B contiguous bytes, the blocks of a range follow each other -- and merges them in tree
//             order: every lane has B - 1 compressions, no LDS, no barrier.  A range of one block is finished here (one leaf: no
//             merge, the leaf's value already carries ROOT); of the others each block's node goes to LDS and the left children of
//             the first level onto a list
//   levels    strides of 1, 2, 4 .. blocks: lane i takes the list's i-th merge, and its node goes onto the next level's list if
//             it is a left child there too, so no level looks at more than the level before it produced.  One barrier per level.
// LDS: the tables (6 bytes a range) and behind them the nodes (32 bytes each) in one array of b3s_max_bytes, two lists of PW_NODES / 2
// entries: 36 KiB, and 60 registers, so FOUR workgroups are resident per CU, 32 waves, all a CU holds.  The kernel is bound by the
// latency of its own chain (five dependent loads before the first compression, then one compression per level with ever fewer
// lanes), which only other workgroups on the same SIMDs cover: with three per CU it takes 2.03 ms on the 64 GiB tree, with four 1.85.
// run_slot != null: the leaves' chaining values are not in the dense leaf order but where the walking scan that hashes left them, range
// c's at slot run_slot[c] of cvs and following (k_blake3_run_slots): one more dependent load per block, and no pass that moves 32 bytes
// a leaf.  (One kernel for both, told apart by the pointer: tests/test_k3_parents_budget.py holds the product to one reducer.)
__global__ __launch_bounds__(PW_THREADS, PW_WAVES) void k_blake3_parents_window(const uint32_t* __restrict__ leaf_prefix, uint64_t count_bound,
                                                                         const uint32_t* __restrict__ n_dev, const uint32_t* __restrict__ cvs,
                                                                         const uint32_t* __restrict__ win_first, uint64_t* __restrict__ hashes,
                                                                         const uint32_t* __restrict__ run_slot)
{
    __shared__ uint4 s_mem[PW_MEM16]; // the tables, behind them the nodes
    __shared__ uint32_t s_list[2][PW_NODES / 2 + 1];                   // node | block inside the range << 16 | blocks of the range << 24
    __shared__ uint32_t s_cnt[PW_LEVELS + 1];
    __shared__ uint32_t s_wsum[PW_THREADS / 64];
    const uint32_t count = (uint32_t)(n_dev ? (*n_dev < count_bound ? *n_dev : count_bound) : count_bound);
    const uint32_t total = leaf_prefix[count];
    const uint64_t w0 = (uint64_t)blockIdx.x * PW;
    if (w0 >= total)
        return;
    const uint32_t tid = threadIdx.x;
    const int lane = (int)(tid & 63u);
    // first range that starts at or after the window / the next window: noted by the leaf kernel's thread of that slot (a
    // binary search here would be ~40 dependent loads before the workgroup can start)
    const uint32_t c_lo = win_first[blockIdx.x];
    const uint32_t c_hi = w0 + PW >= total ? count : win_first[blockIdx.x + 1u];
    const uint32_t nch = c_hi - c_lo;
    if (nch == 0)
        return;
    const uint32_t wbase = leaf_prefix[c_lo];
    if (nch > (uint32_t)PW || leaf_prefix[c_hi] - wbase > (uint32_t)(PW + PW_MAXN - 1))
        return; // not a window of ranges of at most 256 leaves: the tables are not made for it
    if (tid <= PW_LEVELS)
        s_cnt[tid] = 0;
    uint16_t* s_leaf = reinterpret_cast<uint16_t*>(s_mem); // of the window's j-th range: first leaf slot, ..
    uint16_t* s_blk = s_leaf + (nch + 1u);                 // .. first block ..
    uint16_t* s_node = s_blk + (nch + 1u);                 // .. and first node (j = nch: the totals)
    uint4* s_cv = s_mem + (6u * (nch + 1u) + 15u) / 16u;

    // tables: thread t has ranges t R .. t R + R - 1; blocks and nodes are summed in one word (blocks < 2^16)
    constexpr uint32_t R = (PW + PW_THREADS - 1) / PW_THREADS;
    {
        const uint32_t j0 = tid * R;
        uint32_t lp[R + 1], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i <= R; ++i)
            lp[i] = leaf_prefix[c_lo + (j0 + i < nch ? j0 + i : nch)] - wbase;
#pragma unroll
        for (uint32_t i = 0; i < R; ++i)
        {
            const uint32_t n = lp[i + 1] - lp[i], nb = b3s_blocks(n, PB); // (0 behind the window's last range)
            sum += nb | (b3s_to_lds(n, PB) ? nb << 16 : 0u);
        }
        uint32_t incl = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d)
                incl += up;
        }
        if (lane == 63)
            s_wsum[tid >> 6] = incl;
        __syncthreads();
        uint32_t run = incl - sum;
        for (uint32_t w = 0; w < (tid >> 6); ++w)
            run += s_wsum[w];
#pragma unroll
        for (uint32_t i = 0; i <= R; ++i)
        {
            const uint32_t j = j0 + i;
            if (j <= nch && (i < R || j == nch)) // (the entry behind the last range: by whoever reaches it)
            {
                s_leaf[j] = (uint16_t)lp[i];
                s_blk[j] = (uint16_t)(run & 0xFFFFu);
                s_node[j] = (uint16_t)(run >> 16);
            }
            if (i < R)
            {
                const uint32_t n = lp[i + 1] - lp[i], nb = b3s_blocks(n, PB);
                run += nb | (b3s_to_lds(n, PB) ? nb << 16 : 0u);
            }
        }
    }
    __syncthreads();

    if ((6u * (nch + 1u) + 15u) / 16u + 2u * s_node[nch] > PW_MEM16)
        return; // (cannot be: b3s_max_bytes)

    // registers
    const uint32_t nblk = s_blk[nch];
    const uint4* cvs4 = reinterpret_cast<const uint4*>(cvs) + (uint64_t)wbase * 2u;
    for (uint32_t b0 = 0; b0 < nblk; b0 += PW_THREADS)
    {
        const uint32_t blk = b0 + tid;
        bool left = false;
        uint32_t entry = 0;
        if (blk < nblk)
        {
            uint32_t lo = 0, hi = nch; // range j with s_blk[j] <= blk < s_blk[j + 1] (every range has a block)
            while (hi - lo > 1)
            {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (s_blk[mid] <= blk)
                    lo = mid;
                else
                    hi = mid;
            }
            const uint32_t j = lo, b = blk - s_blk[j];
            const uint32_t p = s_leaf[j], n = s_leaf[j + 1] - p, nb = b3s_blocks(n, PB);
            const uint32_t m = b3s_block_leaves(n, b, PB);
            const uint4* g = run_slot ? reinterpret_cast<const uint4*>(cvs) + ((uint64_t)run_slot[c_lo + j] + b * PB) * 2u : cvs4 + (p + b * PB) * 2u;
            uint32_t cv[PB][8];
#pragma unroll
            for (uint32_t i = 0; i < PB; ++i)
            {
                const uint32_t ii = i < m ? i : m - 1u; // (a short block reads its last leaf again: no load is conditional)
                const uint4 x = g[2u * ii], y = g[2u * ii + 1u];
                cv[i][0] = x.x; cv[i][1] = x.y; cv[i][2] = x.z; cv[i][3] = x.w;
                cv[i][4] = y.x; cv[i][5] = y.y; cv[i][6] = y.z; cv[i][7] = y.w;
            }
#pragma unroll
            for (uint32_t st = 1; st < PB; st <<= 1)
            {
#pragma unroll
                for (uint32_t k = 0; k + st < PB; k += 2u * st)
                    if (b3s_reg_merge(m, k, st))
                        b3_merge_regs(cv[k], cv[k + st], (uint32_t)F_PARENT | (b3s_root(n, b * PB + k, st) ? (uint32_t)F_ROOT : 0u));
            }
            if (!b3s_to_lds(n, PB))
                hashes[c_lo + j] = (uint64_t)cv[0][0] | ((uint64_t)cv[0][1] << 32);
            else
            {
                const uint32_t node = (uint32_t)s_node[j] + b;
                s_cv[2u * node] = make_uint4(cv[0][0], cv[0][1], cv[0][2], cv[0][3]);
                s_cv[2u * node + 1u] = make_uint4(cv[0][4], cv[0][5], cv[0][6], cv[0][7]);
                left = b3s_lds_merge(nb, b, 1u);
                entry = node | (b << 16) | (nb << 24);
            }
        }
        pw_append(left, entry, s_list[0], &s_cnt[0], lane);
    }

    // levels
    uint32_t rot = blockIdx.x; // which wave takes the first 64 merges of a level: rotates, or the SIMD of wave 0 does all the thin levels
    for (uint32_t lvl = 0, st = 1;; ++lvl, st <<= 1, ++rot)
    {
        __syncthreads();
        const uint32_t nm = lvl < PW_LEVELS ? s_cnt[lvl] : 0u;
        if (nm == 0)
            break;
        const uint32_t* cur = s_list[lvl & 1u];
        uint32_t* nxt = s_list[(lvl + 1u) & 1u];
        for (uint32_t m0 = 0; m0 < nm; m0 += PW_THREADS)
        {
            const uint32_t mi = m0 + (tid + 64u * rot) % (uint32_t)PW_THREADS;
            bool keep = false;
            uint32_t entry = 0;
            if (mi < nm)
            {
                entry = cur[mi];
                const uint32_t node = entry & 0xFFFFu, k = (entry >> 16) & 0xFFu, nb = entry >> 24;
                const uint4 a0 = s_cv[2u * node], a1 = s_cv[2u * node + 1u];
                const uint4 b0 = s_cv[2u * (node + st)], b1 = s_cv[2u * (node + st) + 1u];
                uint32_t m[16] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                uint32_t cv[8] = {B3_IV0, B3_IV1, B3_IV2, B3_IV3, B3_IV4, B3_IV5, B3_IV6, B3_IV7};
                b3_compress(cv, m, 0u, 64u, (uint32_t)F_PARENT | (b3s_lds_root(nb, st) ? (uint32_t)F_ROOT : 0u));
                s_cv[2u * node] = make_uint4(cv[0], cv[1], cv[2], cv[3]);
                s_cv[2u * node + 1u] = make_uint4(cv[4], cv[5], cv[6], cv[7]);
                keep = b3s_lds_merge(nb, k, 2u * st);
            }
            pw_append(keep, entry, nxt, &s_cnt[lvl + 1u], lane);
        }
    }
    for (uint32_t j = tid; j < nch; j += PW_THREADS)
        if (b3s_to_lds((uint32_t)s_leaf[j + 1] - s_leaf[j], PB))
        {
            const uint4 r = s_cv[2u * s_node[j]];
            hashes[c_lo + j] = (uint64_t)r.x | ((uint64_t)r.y << 32);
        }
}

// big trees: one launch per level, one thread per leaf slot
__global__ __launch_bounds__(256) void k_blake3_parents_level(const uint32_t* __restrict__ leaf_prefix, uint32_t count,
                                                              uint32_t stride, uint32_t* __restrict__ cvs)
{
    const uint32_t total = leaf_prefix[count];
    const uint64_t g64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g64 >= total)
        return;
    const uint32_t g = (uint32_t)g64;
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (leaf_prefix[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    const uint32_t slot0 = leaf_prefix[lo];
    const uint32_t n = leaf_prefix[lo + 1] - slot0;
    const uint32_t k = g - slot0;
    if ((k & ((stride << 1) - 1u)) != 0u || k + stride >= n)
        return;
    const uint32_t last = (stride << 1) >= n;
    b3_parent(cvs + (uint64_t)g * 8u, cvs + (uint64_t)(g + stride) * 8u, (uint32_t)F_PARENT | (last ? (uint32_t)F_ROOT : 0u));
}

__global__ void k_blake3_emit(const uint32_t* __restrict__ leaf_prefix, uint32_t count, const uint32_t* __restrict__ cvs,
                              uint64_t* __restrict__ hashes)
{
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count)
        return;
    const uint32_t* base = cvs + (uint64_t)leaf_prefix[c] * 8u;
    hashes[c] = (uint64_t)base[0] | ((uint64_t)base[1] << 32);
}

// The chaining values that the walking scan hashed itself (k_buzhash.hip) lie in runs, one per part, each filled densely from its
// start in the part's chunk order.  A workgroup per part, behind compaction (which yields leaf_prefix):
//   MOVE   moves the run to the part's place in the dense leaf order -- leaf_prefix of the part's first chunk -- for the reducers that
//          work in place on the dense order (big trees);
//   !MOVE  notes for every chunk of the part the slot of its first leaf in the runs, which k_blake3_parents_window<true> reads them from;
// and both note the windows that start inside the part, as the leaf kernel does.
template <bool MOVE>
__global__ __launch_bounds__(256) void k_blake3_run_slots(const PartDev* __restrict__ parts, uint32_t nparts,
                                                           const uint32_t* __restrict__ part_first,
                                                           const uint32_t* __restrict__ leaf_prefix, const uint4* __restrict__ runs,
                                                           uint4* __restrict__ cvs, uint32_t* __restrict__ run_slot,
                                                           uint32_t* __restrict__ win_first)
{
    const uint32_t p = blockIdx.x;
    if (p >= nparts)
        return;
    const uint32_t c0 = part_first[p], c1 = part_first[p + 1];
    const uint32_t g0 = leaf_prefix[c0], g1 = leaf_prefix[c1];
    if constexpr (MOVE)
    {
        const uint4* src = runs + lthip_part_run_base(parts[p]) * 2u;
        uint4* dst = cvs + (uint64_t)g0 * 2u;
        const uint32_t n = (g1 - g0) * 2u; // (a part is below 4 GiB: its leaves and chunks are below 2^23)
        for (uint32_t i = threadIdx.x; i < n; i += 256u)
            dst[i] = src[i];
    }
    else
    {
        const uint32_t base = (uint32_t)lthip_part_run_base(parts[p]) - g0; // (slots are below 2^32: lthip_launch_buzhash_walk)
        for (uint32_t c = c0 + threadIdx.x; c < c1; c += 256u)
            run_slot[c] = base + leaf_prefix[c];
    }
    if (!win_first)
        return;
    for (uint64_t g = (((uint64_t)g0 + (uint32_t)(PW - 1)) & ~(uint64_t)(PW - 1)) + (uint64_t)threadIdx.x * PW; g < g1; g += 256u * (uint64_t)PW)
    {
        uint32_t lo = c0, hi = c1; // range c of the part with leaf_prefix[c] <= g < leaf_prefix[c + 1]
        while (hi - lo > 1)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (leaf_prefix[mid] <= g)
                lo = mid;
            else
                hi = mid;
        }
        win_first[g / (uint32_t)PW] = leaf_prefix[lo] == g ? lo : lo + 1u;
    }
}

#ifndef B3_RUNS_IN_PLACE
#define B3_RUNS_IN_PLACE 1 // 1: small trees are reduced from the runs of a scan that hashes where they lie; 0: the runs are moved first (profiles/walk_hash_ab.txt)
#endif

} // namespace

static int launch_blake3(lthip_ctx* ctx, const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_lens, const uint32_t* d_count,
                         uint64_t count_bound, uint64_t leaf_bound, uint64_t max_len, uint64_t* d_hashes, const lthip_b3_runs* runs);

int lthip_launch_blake3(lthip_ctx* ctx, const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_lens,
                        const uint32_t* d_count, uint64_t count_bound, uint64_t leaf_bound, uint64_t max_len,
                        uint64_t* d_hashes)
{
    return launch_blake3(ctx, d_data, d_offsets, d_lens, d_count, count_bound, leaf_bound, max_len, d_hashes, nullptr);
}

int lthip_launch_blake3_parents(lthip_ctx* ctx, const lthip_b3_runs& runs, const uint32_t* d_lens, const uint32_t* d_count,
                                uint64_t count_bound, uint64_t leaf_bound, uint64_t max_len, uint64_t* d_hashes)
{
    return launch_blake3(ctx, nullptr, nullptr, d_lens, d_count, count_bound, leaf_bound, max_len, d_hashes, &runs);
}

// runs: the leaves are hashed already and lie in per-part runs; they are moved into place where the leaf kernel would have written them
static int launch_blake3(lthip_ctx* ctx, const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_lens, const uint32_t* d_count,
                         uint64_t count_bound, uint64_t leaf_bound, uint64_t max_len, uint64_t* d_hashes, const lthip_b3_runs* runs)
{
    if (count_bound == 0)
        return 0;
    void *lc, *lp, *cv;
    int err;
    if ((err = lthip_scratch(ctx, S_LEAF_COUNT, (count_bound + 1) * 4, &lc)))
        return err;
    if ((err = lthip_scratch(ctx, S_LEAF_PREFIX, (count_bound + 1) * 4, &lp)))
        return err;
    {
        LaunchTimer t(ctx, LTHIP_K_COMPACT);
        hipLaunchKernelGGL(k_leaf_counts, dim3((uint32_t)div_up_u64(count_bound, 256)), dim3(256), 0, ctx->stream, d_lens,
                           count_bound, d_count, (uint32_t*)lc);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if ((err = lthip_exclusive_scan_u32(ctx, (const uint32_t*)lc, (uint32_t*)lp, count_bound, d_count, LTHIP_K_COMPACT)))
        return err;

    const bool small_trees = max_len != 0 && max_len <= 256u * 1024u;
    uint32_t host_count = 0;
    if (leaf_bound == 0 || !small_trees)
    {
        // need exact numbers on the host: the count (when it lives on the device) and the leaf total
        if (d_count)
        {
            LTHIP_CHECK(ctx, hipMemcpyAsync(&host_count, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
            LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
            if (host_count > count_bound)
                host_count = (uint32_t)count_bound;
        }
        else
            host_count = (uint32_t)count_bound;
        uint32_t total = 0;
        LTHIP_CHECK(ctx, hipMemcpyAsync(&total, (const uint32_t*)lp + host_count, 4, hipMemcpyDeviceToHost, ctx->stream));
        LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
        leaf_bound = total;
        if (host_count == 0)
            return 0;
    }
    if (leaf_bound == 0)
        return 0;
    if (leaf_bound > 0xFFFFFFF0ull)
        return lthip_fail(ctx, EINVAL, "blake3", "too many leaves in one batch");
    if ((err = lthip_scratch(ctx, S_CV, leaf_bound * 32, &cv)))
        return err;
    void* wf = nullptr;
    if (small_trees && (err = lthip_scratch(ctx, S_B3_WINDOWS, (leaf_bound / PW + 2) * 4, &wf)))
        return err;
    LTHIP_ABLATION_ENV(env_serial, "LTHIP_B3_SERIAL_PARENTS"); // one thread per tree (dense order)
    void* slots = nullptr; // small trees are reduced from the runs where they lie
    if (runs && small_trees && B3_RUNS_IN_PLACE && env_serial.get() < 0 &&
        (err = lthip_scratch(ctx, S_CV_SLOTS, (count_bound + 1) * 4, &slots)))
        return err;
    if (runs)
    {
        LaunchTimer t(ctx, LTHIP_K_B3_LEAF);
        if (slots)
            hipLaunchKernelGGL(k_blake3_run_slots<false>, dim3(runs->nparts), dim3(256), 0, ctx->stream, runs->d_parts, runs->nparts,
                               runs->d_part_first, (const uint32_t*)lp, (const uint4*)runs->d_cvs, (uint4*)nullptr, (uint32_t*)slots, (uint32_t*)wf);
        else
            hipLaunchKernelGGL(k_blake3_run_slots<true>, dim3(runs->nparts), dim3(256), 0, ctx->stream, runs->d_parts, runs->nparts,
                               runs->d_part_first, (const uint32_t*)lp, (const uint4*)runs->d_cvs, (uint4*)cv, (uint32_t*)nullptr, (uint32_t*)wf);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    else
    {
        LaunchTimer t(ctx, LTHIP_K_B3_LEAF);
        LTHIP_ABLATION_ENV(env_pad, "LTHIP_B3_PAD_LDS"); // experiment: unused LDS limits the waves per CU
        const int pad_lds = env_pad.get() > 0 ? env_pad.get() : 0;
#ifdef LTHIP_ABLATIONS
        LTHIP_ABLATION_ENV(env_pf, "LTHIP_B3_PREFETCH"); // 0: every block's loads issued and waited for in front of its compression
        if (env_pf.get() == 0)
            hipLaunchKernelGGL(k_blake3_leaves<false>, dim3((uint32_t)div_up_u64(leaf_bound, 256)), dim3(256), (size_t)pad_lds, ctx->stream,
                               d_data, d_offsets, d_lens, (const uint32_t*)lp, count_bound, d_count, (uint32_t*)cv, (uint32_t*)wf);
        else
#endif
            hipLaunchKernelGGL(k_blake3_leaves<true>, dim3((uint32_t)div_up_u64(leaf_bound, 256)), dim3(256), (size_t)pad_lds, ctx->stream,
                               d_data, d_offsets, d_lens, (const uint32_t*)lp, count_bound, d_count, (uint32_t*)cv, (uint32_t*)wf);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if (small_trees)
    {
        LaunchTimer t(ctx, LTHIP_K_B3_PARENT);
#ifdef LTHIP_ABLATIONS
        if (env_serial.get() >= 0)
            hipLaunchKernelGGL(k_blake3_parents_small, dim3((uint32_t)div_up_u64(count_bound, 256)), dim3(256), 0, ctx->stream,
                               d_lens, (const uint32_t*)lp, count_bound, d_count, (uint32_t*)cv, d_hashes);
        else
#endif
            hipLaunchKernelGGL(k_blake3_parents_window, dim3((uint32_t)div_up_u64(leaf_bound, PW)), dim3(PW_THREADS), 0, ctx->stream,
                               (const uint32_t*)lp, count_bound, d_count, slots ? runs->d_cvs : (const uint32_t*)cv, (const uint32_t*)wf, d_hashes,
                               (const uint32_t*)slots);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    else
    {
        LaunchTimer t(ctx, LTHIP_K_B3_PARENT);
        // deepest possible tree: a u32 length has at most 2^22 leaves
        uint64_t max_leaves = max_len ? div_up_u64(max_len, 1024) : (1ull << 22);
        for (uint64_t stride = 1; stride < max_leaves; stride <<= 1)
            hipLaunchKernelGGL(k_blake3_parents_level, dim3((uint32_t)div_up_u64(leaf_bound, 256)), dim3(256), 0,
                               ctx->stream, (const uint32_t*)lp, host_count, (uint32_t)stride, (uint32_t*)cv);
        hipLaunchKernelGGL(k_blake3_emit, dim3((uint32_t)div_up_u64(host_count, 256)), dim3(256), 0, ctx->stream,
                           (const uint32_t*)lp, host_count, (const uint32_t*)cv, d_hashes);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    return 0;
}

// BLAKE3-64 of one input of at most 64 KiB that the device can read where it is (pinned host memory or device memory), result
// written to `out` (pinned host or device): one launch on the context's stream
int lthip_launch_blake3_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out)
{
    if (len > 65536u)
        return lthip_fail(ctx, EINVAL, "blake3_one", "input above 64 KiB");
    LaunchTimer t(ctx, LTHIP_K_B3_LEAF);
    const size_t lds = 64 * 8 * 4 + (size_t)(len ? (len + 1023u) >> 10 : 1u) * B3_ONE_PITCH;
    if (lds > 64u * 1024u)
    {
        static std::atomic<bool> granted[64] = {};
        if (int err = lthip_grant_lds(ctx, granted, {reinterpret_cast<const void*>(&k_blake3_one)}, 80 * 1024))
            return err;
    }
    hipLaunchKernelGGL(k_blake3_one, dim3(1), dim3(64), lds, ctx->stream, (const uint8_t*)in, len, out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

int lthip_launch_blake3_stream_batch(lthip_ctx* ctx, const void* d_data, uint32_t leaf0, uint32_t* d_stack, uint32_t depth_in, uint32_t merges)
{
    LaunchTimer t(ctx, LTHIP_K_B3_LEAF);
    hipLaunchKernelGGL(k_blake3_stream_batch, dim3(1), dim3(B3S_LEAVES), 0, ctx->stream, (const uint8_t*)d_data, leaf0, d_stack, depth_in, merges);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

int lthip_launch_blake3_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint32_t leaf0, const uint32_t* d_stack,
                                     uint32_t depth, uint64_t* d_out)
{
    LaunchTimer t(ctx, LTHIP_K_B3_PARENT);
    hipLaunchKernelGGL(k_blake3_stream_final, dim3(1), dim3(B3S_LEAVES), 0, ctx->stream, (const uint8_t*)d_tail, tail_len, leaf0, d_stack, depth,
                       d_out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}
