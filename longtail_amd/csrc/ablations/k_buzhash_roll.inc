// k_buzhash_roll.inc -- part of k_buzhash.hip, compiled by the ablation build only (-DLTHIP_ABLATIONS, `make ablations`):
// an earlier formulation kept as a second implementation for differential tests and A/B runs; not in the product library.

constexpr int TAB_REP = 64;                  // this kernel's own table: T[v] replicated once per lane, 256 bytes apart: a lookup address is
                                             // {byte, lane * 4} = ONE v_perm_b32 of the data dword, and never conflicts
constexpr int K1_WAVES = 12;                 // one workgroup per CU: 3 waves per SIMD, <= 168 VGPRs each (16 waves at 128 VGPRs spill and gain nothing: measured; the rolling-window kernel)
constexpr int K1_THREADS = 64 * K1_WAVES;
constexpr int WVECS = WROWS * 4;         // 260 16-byte vectors per wave-tile

struct TileRegs
{
    uint4 q[5];
};

__device__ __forceinline__ void tile_load(TileRegs& r, const uint8_t* __restrict__ data, const PartDev& pd,
                                          uint64_t span_start, int lane)
{
    const uint8_t* src = data + pd.off;
#pragma unroll
    for (int u = 0; u < 5; ++u)
    {
        const int v = lane + u * 64;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (v < WVECS)
        {
            const int64_t g = (int64_t)span_start - 64 + 16 * (int64_t)v;
            if (g >= 0)
            {
                if ((uint64_t)g + 16 <= pd.size)
                    q = *reinterpret_cast<const uint4*>(src + g);
                else if ((uint64_t)g < pd.size)
                {
                    uint32_t w[4] = {0, 0, 0, 0};
                    const uint32_t n = (uint32_t)(pd.size - (uint64_t)g);
                    for (uint32_t b = 0; b < n; ++b)
                        w[b >> 2] |= (uint32_t)src[g + b] << (8 * (b & 3));
                    q = make_uint4(w[0], w[1], w[2], w[3]);
                }
            }
        }
        r.q[u] = q;
    }
}

__device__ __forceinline__ void tile_store(const TileRegs& r, uint32_t* __restrict__ rows, int lane)
{
#pragma unroll
    for (int u = 0; u < 5; ++u)
    {
        const int v = lane + u * 64;
        if (v < WVECS)
        {
            uint32_t* d = rows + (v >> 2) * ROW_DW + (v & 3) * 4;
            d[0] = r.q[u].x;
            d[1] = r.q[u].y;
            d[2] = r.q[u].z;
            d[3] = r.q[u].w;
        }
    }
}

template <int MODE> // 0 = general d (multiply test), 1 = power-of-two d (mask test)
__global__ __launch_bounds__(K1_THREADS, 1) void k_buzhash_candidates(const uint8_t* __restrict__ data,
                                                                       const PartDev* __restrict__ parts,
                                                                       const uint32_t* __restrict__ tile_part,
                                                                       uint32_t ntiles, DivTest dv,
                                                                       uint64_t* __restrict__ bm0,
                                                                       uint64_t* __restrict__ bm1)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* tab = smem; // [256][TAB_REP]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6); // provably wave-uniform: tile bookkeeping stays in SGPRs
    uint32_t* rows = smem + 256 * TAB_REP + wave * (WROWS * ROW_DW); // this wave's [WROWS][ROW_DW]

    // replicated substitution table: tab[v*TAB_REP + r] = T[v]
    if (tid < 256)
    {
        const uint32_t tv = c_buztab[tid];
        uint4 q = make_uint4(tv, tv, tv, tv);
        uint4* dst = reinterpret_cast<uint4*>(tab + tid * TAB_REP);
#pragma unroll
        for (int j = 0; j < TAB_REP / 4; ++j)
            dst[j] = q;
    }
    __syncthreads(); // the only barrier: table visible to every wave
    // The table is the first thing in LDS and the kernel has no static LDS, so its LDS address is 0 and a lookup address
    // is the v_perm result itself (no base add); checked, not assumed.
    if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)smem != 0u)
        __builtin_trap();
    const uint32_t lane4 = (uint32_t)lane * 4u;
    // x divisible by odd d' <=> x * d'^-1 mod 2^32 <= (2^32-1)/d'
    const uint32_t qodd = MODE == 1 ? 0u : 0xFFFFFFFFu / (dv.d >> dv.k2);

    const uint64_t nwt = (uint64_t)ntiles * 4u; // wave-tiles; wave-tile wt is quarter (wt & 3) of 16 KiB tile (wt >> 2)
    const uint64_t wstride = (uint64_t)gridDim.x * (uint64_t)K1_WAVES;
    uint64_t wt = (uint64_t)blockIdx.x * (uint64_t)K1_WAVES + (uint64_t)wave;
    if (wt >= nwt)
        return;
    PartDev pd = parts[tile_part[wt >> 2]];
    uint64_t span = ((wt >> 2) - pd.tile_base) * (uint64_t)TILE + (wt & 3u) * (uint64_t)WTILE; // part-relative
    TileRegs regs;
    tile_load(regs, data, pd, span, lane);

    for (;;)
    {
        __builtin_amdgcn_wave_barrier();
        tile_store(regs, rows, lane);
        __builtin_amdgcn_wave_barrier();

        // issue the next wave-tile's global loads now; they land while this one is being hashed
        const uint64_t next = wt + wstride;
        PartDev npd = pd;
        uint64_t next_span = 0;
        if (next < nwt)
        {
            npd = parts[tile_part[next >> 2]];
            next_span = ((next >> 2) - npd.tile_base) * (uint64_t)TILE + (next & 3u) * (uint64_t)WTILE;
            tile_load(regs, data, npd, next_span, lane);
        }

        const uint64_t q0 = span + (uint64_t)lane * RUN; // first byte of my run
        uint32_t mlo = 0, mhi = 0;
        if (q0 < pd.size)
        {
            // window bytes: j in [0,112): j<48 = the 48 bytes before the run, j>=48 = the run
            uint32_t win[28];
            const uint32_t* prev = rows + lane * ROW_DW;
#pragma unroll
            for (int i = 0; i < 12; ++i)
                win[i] = prev[4 + i];
#pragma unroll
            for (int i = 0; i < 16; ++i)
                win[12 + i] = prev[ROW_DW + i];

            // T[byte] of the window bytes is fetched in two batches of independent LDS reads (80 + 32) that stream
            // through the LDS pipe back to back, each followed by pure register arithmetic.  The value that enters
            // the hash at step k leaves it at step k+48 (hpcdcchunker.c:294-296; rotl(T[out], 48 & 31)).
            uint32_t tv[48 + RUN];
            uint32_t h = 0;
    // byte offset of T[b] for this lane = b * 256 + lane * 4 = bytes {lane4, b, 0, 0}
#define LT_LOOKUP(j)                                                                                                 \
    tv[j] = lds_load_u32(__builtin_amdgcn_perm(win[(j) >> 2], lane4, 0x0c0c0400u | ((uint32_t)((j) & 3) << 8)))
#define LT_STEP(k)                                                                                                   \
    {                                                                                                                \
        h = rotl32(h, 1) ^ rotl32(tv[k], 16) ^ tv[48 + (k)];                                                         \
        bool pre;                                                                                                    \
        if (MODE == 1)                                                                                               \
            pre = (h & (dv.d - 1u)) == dv.d - 1u;                                                                    \
        else /* necessary: the odd part of d divides h+1 (3 ops); the exact test waits in the rare branch */        \
            pre = h * dv.inv + dv.inv <= qodd;                                                                       \
        if (__builtin_amdgcn_ballot_w64(pre) != 0ull) /* wave-uniform and rare (1 position in d's odd part) */       \
        {                                                                                                            \
            asm volatile(""); /* keep this a real scalar branch (no if-conversion of the bit-set) */                 \
            const bool hit = MODE == 1 ? pre : rotr32(h * dv.inv + dv.addc, dv.k2) <= dv.qlim; /* h % d == d-1 */   \
            /* 0/1 shifted by an inline constant: a select between 0 and 1 << k would park 64 constants in VGPRs */ \
            uint32_t hb;                                                                                             \
            asm volatile("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(hb) : "s"(__builtin_amdgcn_ballot_w64(hit)));       \
            if ((k) < 32)                                                                                            \
                mlo |= hb << (k);                                                                                    \
            else                                                                                                     \
                mhi |= hb << ((k)-32);                                                                               \
        }                                                                                                            \
    }
#pragma unroll
            for (int j = 0; j < 80; ++j)
                LT_LOOKUP(j);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 48; ++j)
                h = rotl32(h, 1) ^ tv[j];
#pragma unroll
            for (int k = 0; k < 32; ++k)
                LT_STEP(k)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 80; j < 48 + RUN; ++j)
                LT_LOOKUP(j);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 32; k < RUN; ++k)
                LT_STEP(k)
#undef LT_LOOKUP
#undef LT_STEP
            // bit k <=> cut position p = q0+k+1 ; legal cuts are 48 <= p <= size
            uint64_t m = ((uint64_t)mhi << 32) | mlo;
            if (q0 < 47)
                m &= ~0ull << (47 - q0);
            const uint64_t remain = pd.size - q0; // >= 1
            if (remain < 64)
                m &= (1ull << remain) - 1ull;
            mlo = (uint32_t)m;
            mhi = (uint32_t)(m >> 32);
        }
        const uint64_t m = ((uint64_t)mhi << 32) | mlo;
        const uint64_t summary = __builtin_amdgcn_ballot_w64(m != 0ull);
        if (m != 0ull)
            bm0[pd.bm0_base + (span >> 6) + (uint64_t)lane] = m; // one word per 64-byte run
        if (lane == 0)
            bm1[pd.bm1_base + (span >> 12)] = summary;            // one word per 4 KiB

        if (next >= nwt)
            break;
        wt = next;
        pd = npd;
        span = next_span;
    }
}
