// lz4_stitch.inc -- part of k_lz4.hip (one translation unit; included there, inside its anonymous namespace, in this order):
// K6: per-block scan of the units' results into exact output offsets (k_lz4_stitch_scan) and the copy into the final block (k_lz4_stitch_copy)
__device__ __forceinline__ void wg_emit_header(uint8_t* dst, uint32_t lits, uint32_t match_nibble, int tid, int nthreads)
{
    if (tid == 0)
        dst[0] = (uint8_t)(((lits < 15u ? lits : 15u) << 4) | match_nibble);
    if (lits >= 15u)
    {
        const uint32_t len = lits - 15u;
        const uint32_t n = len / 255u + 1u;
        for (uint32_t j = tid; j < n; j += nthreads)
            dst[1 + j] = j + 1 == n ? (uint8_t)(len % 255u) : (uint8_t)255;
    }
}

// ---------------------------------------------------------------------------------------------------
// K6a: per-block serial walk over segment results
// ---------------------------------------------------------------------------------------------------
// One wave per block.  The walk over the units is inherently serial (a unit's placement depends on the literal
// carry of its predecessors) but its inputs are not: 64 result records are loaded per step with one coalesced
// load, the serial logic then runs wave-uniformly on readlane'd values, and the placement records are stored
// coalesced again.  Trailing literals belong to a literal RUN that is closed by the next unit with a match (or by
// the end of the block); the start of a run's literal area is only known when it closes, so units remember
// (run index, offset inside the run) and k_lz4_stitch_copy resolves it through the run table.
__global__ __launch_bounds__(64) void k_lz4_stitch_scan(const Lz4Block* __restrict__ blocks, uint32_t b0, uint32_t nblocks, uint32_t SEG,
                                                        const Lz4Meta* __restrict__ meta, Lz4Plan* __restrict__ plan,
                                                        uint32_t* __restrict__ runs, Lz4BlockOut* __restrict__ bout,
                                                        uint32_t* __restrict__ out_sizes, uint8_t* __restrict__ dst, uint32_t spec,
                                                        uint32_t* __restrict__ worklist /* from [1]: group ids, then (from 1 + wl_cap) their blocks */,
                                                        uint32_t wl_cap, uint32_t* wl_count /* how many */,
                                                        const uint32_t* seq_units /* lz4_seq_units, or null: every block is walked */)
{
    const uint32_t b = blockIdx.x + b0;
    if (b >= nblocks)
        return;
    const int lane = threadIdx.x;
    const Lz4Block blk = blocks[b];
    const uint32_t run_base = blk.seg_base + b; // this block's slice of the run table (<= nseg + 1 runs)
    uint64_t out_pos = 0; // 64-bit: pathological inputs are caught against dst_cap at the end
    uint32_t carry = 0;
    uint32_t run = 0;
    // A block none of whose units holds a sequence (incompressible data) was laid out by the match finder (spec) and is one literal run:
    // what the walk would end with -- no run closed, nothing put out, every byte carried -- is known without it, and its units' records
    // are not even loaded.  Such a block's plan[] is not written; nobody reads it (the copy kernel visits listed groups only).
    const bool plain = seq_units && spec && blk.nseg != 0u && seq_units[blk.grp_base] == 0u;
    const uint32_t nwalk = plain ? 0u : blk.nseg;
    if (plain)
        carry = blk.size;
    // The walk is a recurrence over (literal carry, output position, run count), restated as three wave scans per 64
    // units so that no step is serial:  a unit WITH a match resets the carry to its tail literals, one without adds its
    // length (segmented inclusive scan);  only units with a match advance the output (prefix sum of token + length
    // bytes + literals + body, all functions of the carry that reaches them) and close a run (prefix count).
    Lz4Meta m;
    m.seq_bytes = m.tail_lits = m.first_lit_len = m.first_hdr_bytes = 0;
    if ((uint32_t)lane < nwalk)
        m = meta[blk.seg_base + (uint32_t)lane];
    for (uint32_t i0 = 0; i0 < nwalk; i0 += 64)
    {
        const uint32_t i = i0 + (uint32_t)lane;
        const Lz4Meta cur = m;
        if (i + 64u < blk.nseg) // next step's records are in flight while this one is scanned
            m = meta[blk.seg_base + i + 64u];
        const bool valid = i < blk.nseg;
        const bool has = valid && cur.seq_bytes != 0u;
        const uint32_t seg_len = valid ? (blk.size - i * SEG < SEG ? blk.size - i * SEG : SEG) : 0u;
        // inclusive segmented scan of the carry each unit leaves behind
        uint32_t sv = has ? cur.tail_lits : seg_len;
        uint32_t sf = has ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint32_t pv = __shfl_up(sv, d, 64);
            const uint32_t pf = __shfl_up(sf, d, 64);
            if (lane >= d)
            {
                if (!sf)
                    sv += pv;
                sf |= pf;
            }
        }
        if (!sf)
            sv += carry; // nobody before me in this step had a match: the carry of the previous steps reaches me
        uint32_t cin = __shfl_up(sv, 1, 64); // the carry that reaches me
        if (lane == 0)
            cin = carry;
        // output advance of the units with a match
        const uint32_t L = cin + cur.first_lit_len;
        const uint32_t hdr = 1u + lz4_len_bytes(L);
        const uint64_t adv = has ? (uint64_t)hdr + L + (cur.seq_bytes - cur.first_hdr_bytes - cur.first_lit_len) : 0ull;
        uint64_t pos = adv; // inclusive prefix sum
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const uint64_t pv = __shfl_up(pos, d, 64);
            if (lane >= d)
                pos += pv;
        }
        const uint64_t my_pos = out_pos + pos - adv;
        const uint64_t hm = __builtin_amdgcn_ballot_w64(has);
        const uint32_t before = (uint32_t)__builtin_popcountll(hm & ((1ull << lane) - 1ull));
        Lz4Plan pl;
        pl.hdr_pos = 0xFFFFFFFFu;
        pl.hdr_lits = pl.first_lit_dst = pl.body_dst = 0;
        pl.tail_rel = cin;
        pl.run = run_base + run + before;
        if (has)
        {
            const uint64_t lit_dst = my_pos + hdr;
            runs[run_base + run + before] = (uint32_t)lit_dst; // closes the open run
            pl.hdr_pos = (uint32_t)my_pos;
            pl.hdr_lits = L;
            pl.first_lit_dst = (uint32_t)(lit_dst + cin);
            pl.body_dst = pl.first_lit_dst + cur.first_lit_len;
            pl.tail_rel = 0; // this unit's tail opens the next run
            pl.run = run_base + run + before + 1u;
        }
        if (valid)
            plan[blk.seg_base + i] = pl;
        out_pos += __shfl(pos, 63, 64);
        carry = __shfl(sv, 63, 64); // lanes past the end add nothing
        run += (uint32_t)__builtin_popcountll(hm);
    }
    // final literal-only sequence (lz4.c:1302-1329)
    const uint32_t hdr = 1u + lz4_len_bytes(carry);
    const uint64_t lit_dst = out_pos + hdr;
    const uint64_t total = lit_dst + carry;
    // Which groups does the copy kernel have to visit?  A block without a single match was laid out by the match finder
    // (spec): its one header is written here and the copy kernel never hears of it.
    if (total <= (uint64_t)blk.dst_cap)
    {
        if (run == 0u && spec)
        {
            if (blk.nseg)
                wg_emit_header(dst + blk.dst_off + out_pos, carry, 0u, lane, 64);
        }
        else
        {
            uint32_t base = 0;
            if (lane == 0)
                base = atomicAdd(wl_count, blk.ngrp);
            base = __builtin_amdgcn_readfirstlane(base);
            for (uint32_t k = lane; k < blk.ngrp; k += 64)
            {
                worklist[1u + base + k] = blk.grp_base + k;
                worklist[1u + wl_cap + base + k] = b; // (the copy kernel used to search the block table for it: ten dependent loads per group)
            }
        }
    }
    if (lane == 0)
    {
        runs[run_base + run] = (uint32_t)lit_dst;
        Lz4BlockOut bo;
        bo.final_hdr_pos = (uint32_t)out_pos;
        bo.final_lits = carry;
        bo.total = total <= (uint64_t)blk.dst_cap ? (uint32_t)total : 0u;
        bo.pad = run == 0u ? 1u : 0u; // no unit found a match: the literals were placed by the match finder already
        bout[b] = bo;
        out_sizes[b] = bo.total;
    }
}

// ---------------------------------------------------------------------------------------------------
// K6b: one workgroup per segment moves its pieces into place
// ---------------------------------------------------------------------------------------------------
// a wave copies n bytes (k_copy.h)
__device__ __forceinline__ void wg_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t n, int lane)
{
    if (n)
        lthip_wg_copy<64>(dst, src, n, lane);
}

constexpr int K6_THREADS = 256;

// one workgroup per window group: its (up to gunits) units are moved into place one after the other
#ifdef LTHIP_K6_WAVES
__attribute__((amdgpu_waves_per_eu(LTHIP_K6_WAVES, LTHIP_K6_WAVES)))
#endif
__global__ __launch_bounds__(K6_THREADS) void k_lz4_stitch_copy(const uint8_t* __restrict__ src,
                                                                 const Lz4Block* __restrict__ blocks, uint32_t nblocks,
                                                                 uint32_t SEG, const uint8_t* __restrict__ streams,
                                                                 const Lz4Meta* __restrict__ meta,
                                                                 const Lz4Plan* __restrict__ plan,
                                                                 const uint32_t* __restrict__ runs,
                                                                 const Lz4BlockOut* __restrict__ bout,
                                                                 uint8_t* __restrict__ dst, const uint32_t* __restrict__ worklist,
                                                                 uint32_t gunits /* units per window group */, uint32_t wl_cap,
                                                                 const uint32_t* __restrict__ wl_count)
{
    // nothing listed (no block of the batch has a match): every workgroup leaves on this one scalar load
    const uint32_t nwork = *wl_count;
    if (nwork == 0u)
        return;
    const int tid = threadIdx.x;
    (void)nblocks;
  for (uint32_t wi = blockIdx.x; wi < nwork; wi += gridDim.x)
  {
    const uint32_t grp = worklist[1u + wi];
    const uint32_t lo = worklist[1u + wl_cap + wi]; // the group's block (k_lz4_stitch_scan)
    const Lz4Block blk = blocks[lo];
    const Lz4BlockOut bo = bout[lo];
    uint8_t* d = dst + blk.dst_off;
    const uint32_t i0 = (grp - blk.grp_base) * gunits;
    const uint32_t i1 = i0 + gunits < blk.nseg ? i0 + gunits : blk.nseg;
    // each wave moves whole units on its own (4 units in flight per workgroup: their table loads overlap)
    const int lane = tid & 63;
    for (uint32_t i = i0 + (uint32_t)(tid >> 6); i < i1; i += K6_THREADS / 64)
    {
        const uint32_t seg = blk.seg_base + i;
        const uint32_t seg_start = i * SEG;
        const uint32_t len = blk.size - seg_start < SEG ? blk.size - seg_start : SEG;
        const Lz4Meta m = meta[seg];
        const Lz4Plan pl = plan[seg];
        const uint8_t* s = src + blk.src_off + seg_start;
        const uint8_t* stream = streams + (uint64_t)seg * lz4_stream_stride(SEG);
        uint32_t tail = len;
        if (m.seq_bytes)
        {
            wg_emit_header(d + pl.hdr_pos, pl.hdr_lits, stream[0] & 15u, lane, 64);
            wg_copy(d + pl.first_lit_dst, s, m.first_lit_len, lane);
            const uint32_t skip = m.first_hdr_bytes + m.first_lit_len;
            wg_copy(d + pl.body_dst, stream + skip, m.seq_bytes - skip, lane);
            tail = m.tail_lits;
        }
        wg_copy(d + runs[pl.run] + pl.tail_rel, s + (len - tail), tail, lane);
        if (i + 1 == blk.nseg)
            wg_emit_header(d + bo.final_hdr_pos, bo.final_lits, 0u, lane, 64);
    }
  }
}

// empty blocks have no segment: their single 0x00 token is written here
__global__ void k_lz4_empty_blocks(const Lz4Block* __restrict__ blocks, uint32_t nblocks,
                                   const Lz4BlockOut* __restrict__ bout, uint8_t* __restrict__ dst)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nblocks)
        return;
    if (blocks[b].nseg == 0 && bout[b].total == 1)
        dst[blocks[b].dst_off] = 0;
}
