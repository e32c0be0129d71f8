// k_buzhash_prefix_regs.inc -- part of k_buzhash.hip, compiled by the ablation build only (-DLTHIP_ABLATIONS, `make ablations`):
// an earlier formulation kept as a second implementation for differential tests and A/B runs; not in the product library.

// Flavour 1: wave-tiles staged through registers into padded rows (the round-1/2 loader).
template <int MODE, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_buzhash_prefix(const uint8_t* __restrict__ data,
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
    uint32_t* rows = smem + TAB_DW + wave * (WROWS * ROW_DW + HALO_DW); // this wave's [WROWS][ROW_DW] + halo suffixes
    uint32_t* halo = rows + WROWS * ROW_DW;
    prefix_table_init(smem, tid, 64 * WAVES);

    const uint32_t rows_byte = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)rows;
    PrefixConsts pc;
    pc.hj = 63u - (uint32_t)lane;
    pc.halo_byte = rows_byte + WROWS * ROW_DW * 4u;
    pc.thr = MODE == 1 ? 0u : 0xFFFFFFFFu / (dv.d >> dv.k2);
    pc.exact_add = dv.addc - dv.inv;

    const uint64_t nwt = (uint64_t)ntiles * 4u;
    const uint64_t wstride = (uint64_t)gridDim.x * (uint64_t)WAVES;
    uint64_t wt = (uint64_t)blockIdx.x * (uint64_t)WAVES + (uint64_t)wave;
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

        const uint64_t next = wt + wstride;
        PartDev npd = pd;
        uint64_t next_span = 0;
        if (next < nwt)
        {
            npd = parts[tile_part[next >> 2]];
            next_span = ((next >> 2) - npd.tile_base) * (uint64_t)TILE + (next & 3u) * (uint64_t)WTILE;
            tile_load(regs, data, npd, next_span, lane);
        }

        uint32_t win[16];
        const uint32_t* own = rows + (lane + 1) * ROW_DW;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            win[i] = own[i];
        const uint32_t hb = lds_load_u8(rows_byte + pc.hj); // row 0 = the halo row
        const uint64_t m = prefix_legal(prefix_tile<MODE>(win, hb, pc, dv, lane, halo), span + (uint64_t)lane * RUN, pd.size);

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
