// lz4_lanes_kernel.inc -- part of k_lz4.hip (one translation unit; included there, inside its anonymous namespace, in this order):
// K5 pass 2: the list of half-group items (k_lz4_pair_halves) and the persistent lane-parser kernel over it (k_lz4_lanes2)

// ---------------------------------------------------------------------------------------------------
// K5 lane parser, round 4: HALF-GROUPS as the unit of work.  The classification pass flags redundancy per 32 KiB half of a 64 KiB
// group; a group with one redundant and one incompressible half (37 % of the listed groups of bench.py's compressible tree: regions
// of four kinds, a quarter of them random, at arbitrary offsets against the groups) kept eight of the workgroup's sixteen waves idle
// for the whole group.  Now the list is turned into ITEMS of two halves: the two halves of a group that is redundant throughout
// (linked: one contiguous 64 KiB window, as before), or two LONE halves of different groups, which share nothing but the workgroup --
// each has its own 32 KiB of the window (candidates below a half's start are refused), its own half of the shared table, its own
// source alignment.  What a half compresses to does not depend on its partner.
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t LZ4_HALF_NONE = 0xFFFFFFFFu;
constexpr uint32_t LZ4_HALF_HIST = 0x40000000u; // on an item's first half: staged as HISTORY of the second, not parsed (k_lz4_pair_halves, hist)
// worklist layout behind the classification pass (ngroups = groups of the batch): [0 .. ngroups] the blocks' counts of units with a
// sequence and the stitch's work count (k_lz4.hip, lz4_seq_units), [1 + ngroups ..) per-group half bits, [2 ngroups + 1] ticket, [2 ngroups + 2] items, [2 ngroups + 3] lone halves,
// [2 ngroups + 4 ..) items of four words {half a, half b, block of a, block of b} (up to two per group), [10 ngroups + 4 ..) lone halves
__host__ __device__ constexpr uint32_t lz4_items_off(uint32_t ngroups) { return (2u * ngroups + 4u + 3u) & ~3u; } // (16-byte aligned: items are read as uint4)
__device__ __forceinline__ uint32_t lz4_block_of_group(const Lz4Block* __restrict__ blocks, uint32_t nblocks, uint32_t grp)
{
    uint32_t lo = 0, hi = nblocks;
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (blocks[mid].grp_base <= grp)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
// hist (the zstd flavour's "high" and "max" settings): every flagged half becomes an item of its own whose OTHER half is the 32 KiB in
// front of it, staged as history and not parsed -- a half's matches then reach 32 .. 64 KiB back wherever the half lies in its group
// (a lower half has no history otherwise, and an upper half only when the lower one is flagged too), at the price of eight idle waves
// per item.  The first half of every 128 KiB PIECE takes no history: the frame's pieces stay independent (k_zstd.hip decodes them
// with a wave each).
__global__ void k_lz4_pair_halves(uint32_t* __restrict__ wl, uint32_t ngroups, uint32_t phase, const Lz4Block* __restrict__ blocks, uint32_t nblocks,
                                  uint32_t hist)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t* items = wl + lz4_items_off(ngroups);
    uint32_t* lone = items + 8u * ngroups;
    if (phase == 0u)
    {
        // every group of the batch: which of its halves did the classification pass note?
        if (i >= ngroups)
            return;
        const uint32_t g = i, bits = wl[1u + ngroups + g] & 3u;
        if (bits == 0u)
            return;
        if (hist)
        {
            const uint32_t b = lz4_block_of_group(blocks, nblocks, g);
            // (a piece = two groups; hist 3 -- the "max" setting -- lets a piece's first half see the piece before, except every
            // LZ4_Z_CHAIN-th piece of the block: the decoder runs the pieces in between as a chain, k_zstd.hip)
            const bool piece_first = hist == 3u ? ((g - blocks[b].grp_base) % (2u * LZ4_Z_CHAIN)) == 0u : ((g - blocks[b].grp_base) & 1u) == 0u;
            for (uint32_t hh = 0; hh < 2u; ++hh)
                if ((bits >> hh) & 1u)
                {
                    const uint32_t h = 2u * g + hh;
                    if (hh == 0u && piece_first)
                        lone[atomicAdd(&wl[2u * ngroups + 3u], 1u)] = h;
                    else
                    {
                        const uint32_t k = atomicAdd(&wl[2u * ngroups + 2u], 1u);
                        items[4u * k] = (h - 1u) | LZ4_HALF_HIST;
                        items[4u * k + 1u] = h;
                        items[4u * k + 2u] = b;
                        items[4u * k + 3u] = b;
                    }
                }
        }
        else if (bits == 3u)
        {
            const uint32_t k = atomicAdd(&wl[2u * ngroups + 2u], 1u);
            const uint32_t b = lz4_block_of_group(blocks, nblocks, g); // (the ten dependent loads of the search happen here, once, in parallel)
            items[4u * k] = 2u * g;
            items[4u * k + 1u] = 2u * g + 1u;
            items[4u * k + 2u] = b;
            items[4u * k + 3u] = b;
        }
        else if (bits)
            lone[atomicAdd(&wl[2u * ngroups + 3u], 1u)] = 2u * g + (bits >> 1);
    }
    else
    {
        const uint32_t nl = wl[2u * ngroups + 3u];
        if (2u * i >= nl)
            return;
        const uint32_t k = atomicAdd(&wl[2u * ngroups + 2u], 1u);
        const uint32_t a = lone[2u * i], b = 2u * i + 1u < nl ? lone[2u * i + 1u] : LZ4_HALF_NONE;
        items[4u * k] = a;
        items[4u * k + 1u] = b;
        items[4u * k + 2u] = lz4_block_of_group(blocks, nblocks, a >> 1);
        items[4u * k + 3u] = b != LZ4_HALF_NONE ? lz4_block_of_group(blocks, nblocks, b >> 1) : 0u;
    }
}

// Sixteen waves per workgroup: an item of two halves per workgroup, one workgroup per CU.
template <int FMT>
__global__ __launch_bounds__(64 * LZ4_G_LANES, 4) void k_lz4_lanes2(const uint8_t* __restrict__ src, const Lz4Block* __restrict__ blocks, uint32_t nblocks,
                                                       uint32_t sub_bytes, uint8_t* __restrict__ streams, Lz4Meta* __restrict__ meta,
                                                       uint64_t* __restrict__ zrecs, uint8_t* __restrict__ spec_dst, uint32_t dbg,
                                                       uint32_t ngroups, uint32_t* __restrict__ worklist, uint32_t farlog)
{
    constexpr int G = LZ4_G_LANES, TAB = LZ4_TAB_SHARED, SH = LZ4_SH_LOG2;
    // no item (incompressible data): every wave leaves on this one scalar load, before any LDS access and any barrier
    const uint32_t nitems = worklist[2u * ngroups + 2u];
    if (nitems == 0u)
        return;
    const uint32_t far1 = 1u << (farlog & 31u), far2 = 1u << ((farlog >> 8) & 31u), far3 = (farlog >> 16) & 255u; // (zstd flavour: lz4_lane_parse2; far3 = bytes a match into the history half must have)
    constexpr bool PAD = true;
    constexpr uint32_t GAP = 32u; // LDS bytes between the windows of two unlinked halves
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const uint32_t data_bytes = lz4_window_lds_bytes((uint32_t)G * sub_bytes + 64u + LZ4_LPAD + GAP, true);
    uint32_t* sdata = smem;
    lds_window_must_start_at_zero(sdata);
    uint32_t* flag = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(smem) + data_bytes); // 16 bytes
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t hsel = (uint32_t)wave >> 3, wih = (uint32_t)wave & 7u; // my half of the item, my unit in the half
    uint16_t* tab = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(smem) + data_bytes + 16u) + (size_t)wave * TAB;
    uint32_t* shr = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(smem) + data_bytes + 16u + (size_t)G * TAB * 2);
    constexpr uint32_t SH_BYTES = 4u << SH;
    const uint32_t* items = worklist + lz4_items_off(ngroups);
    const uint32_t half_bytes = (uint32_t)(G / 2) * sub_bytes;
    K5P_DECL
    uint32_t sh_gen = 0;
    uint32_t next_idx = 0;
    // (Fetching the next item's lines into registers during the parse -- 16 VGPRs -- was built and measured in round 4 as in round 3:
    // no difference, 4.24 / 4.08 / 6.03 ms with it against 4.23 / 4.06 / 6.00 without on mixed / records / tokens.  An item's fixed
    // cost is LDS work -- 16 K ds_min_u32, the table clears and preloads -- and two barriers, not the latency of its loads.)
    for (uint32_t idx = blockIdx.x; idx < nitems; idx = next_idx)
    {
        if (sh_gen == 0u)
        {
            uint4* hv = reinterpret_cast<uint4*>(shr);
            const uint4 none = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
            for (uint32_t v = tid; v < SH_BYTES / 16u; v += 64 * G)
                hv[v] = none;
            __syncthreads();
            sh_gen = (dbg & (1u << 26)) ? 3u : 0xFFFFu;
        }
        --sh_gen;
        const uint32_t sh_base = sh_gen << 16;
        const uint4 item = reinterpret_cast<const uint4*>(items)[idx];
        const bool hist = (item.x & LZ4_HALF_HIST) != 0u; // (a first half is never LZ4_HALF_NONE)
        const uint32_t ha = item.x & ~LZ4_HALF_HIST, hb = item.y;
        const bool linked = hist || (hb == ha + 1u && !(ha & 1u)); // one contiguous 64 KiB window
        const uint32_t hid = hsel ? hb : ha;
        const bool valid = hid != LZ4_HALF_NONE;
        const uint32_t grp = valid ? hid >> 1 : ha >> 1, hh = valid ? hid & 1u : 0u;
        const Lz4Block blk = blocks[valid && hsel ? item.w : item.z];
        const uint32_t gi = grp - blk.grp_base;
        const uint32_t half_start = (gi * (uint32_t)G + hh * (uint32_t)(G / 2)) * sub_bytes; // block relative
        const uint32_t hlen = valid && half_start < blk.size ? (blk.size - half_start < half_bytes ? blk.size - half_start : half_bytes) : 0u;
        const uint8_t* g = src + blk.src_off + half_start;
        const uint32_t head_src = (uint32_t)((uintptr_t)g & 15u);
        const uint32_t wbase = hsel * half_bytes;                       // window position of my half's first byte
        const uint32_t extra = hsel && !linked ? GAP : 0u;              // its LDS displacement
        const uint32_t head = head_src + LZ4_LPAD + extra;              // LDS byte address of window position x: x + head
        const uint32_t lo_bound = hsel && !linked ? half_bytes : 0u;
        const bool split = !linked || hist; // every half has its own half of the shared table
        const uint32_t sh_shift = split ? 33u - (uint32_t)SH : 32u - (uint32_t)SH;
        const uint32_t sh_off = split ? hsel << (SH - 1) : 0u;
        const uint32_t sh_inv = hist && hsel == 0u ? 0xFFFFu : 0u; // a history half keeps its LATEST occurrences: positions stored inverted

        // ---- every half is staged by its own eight waves (16-byte loads from the aligned-down address); the aligned dwords enter the
        // half's part of the shared table from the registers that stage them ----
        {
            const uint4* gv = reinterpret_cast<const uint4*>(g - head_src);
            const uint32_t nvec = hlen ? (head_src + hlen + 15u) >> 4 : 0u;
            const uint32_t line0 = (wbase + extra + LZ4_LPAD) >> 4; // LDS line (unpadded numbering) of my half's source line 0
            const uint32_t th = (uint32_t)tid & 511u; // (my thread among the eight waves of my half)
            for (uint32_t v0 = 0; v0 < nvec; v0 += 512u * 4u)
            {
                uint4 q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                {
                    const uint32_t v = v0 + (uint32_t)u * 512u + th;
                    q[u] = v < nvec ? gv[v] : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                {
                    const uint32_t v = v0 + (uint32_t)u * 512u + th;
                    if (v < nvec)
                    {
                        const uint32_t D = 4u * (line0 + v);
                        uint32_t* w = sdata + lds_pidx(D);
                        w[0] = q[u].x;
                        w[1] = q[u].y;
                        w[2] = q[u].z;
                        w[3] = q[u].w;
                        if ((D & 31u) == 0u && D != 0u) // the first line of a row: repeated behind the row before
                        {
                            w[-3] = q[u].x;
                            w[-2] = q[u].y;
                            w[-1] = q[u].z;
                        }
                        const uint32_t pq = wbase + 16u * v - head_src; // window position of the line's first byte
                        const uint32_t g4[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
                        // a dword that an EARLIER dword of the same line repeats cannot lower its slot (the table keeps the minimum):
                        // data of a short period (runs, 8-byte patterns) would otherwise send every lane's four updates to one or two
                        // slots, which the LDS serialises (21 % of the kernel on "lines")
                        // ... and the same for the dword at the same place of the line before (the lane before holds it): zero pages
                        // and other runs leave one update per wave
                        // (all of it unconditional, the truth values combined with | and &: as a chain of || and && the compiler wrapped every
                        // neighbour test into its own exec-mask region -- 28 scalar instructions a line in a phase where all sixteen waves
                        // of the CU queue at its one scalar unit)
                        const bool nb = (lane != 0) & (pq >= wbase + 16u);
                        bool dup[4] = {false, g4[1] == g4[0], (bool)((g4[2] == g4[0]) | (g4[2] == g4[1])), (bool)((g4[3] == g4[1]) | (g4[3] == g4[2]) | (g4[3] == g4[0]))};
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            dup[k] = (bool)(dup[k] | (nb & ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)g4[k], 0x138 /* wave_shr:1 */, 0xf, 0xf, true) == g4[k])));
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                        {
                            const uint32_t pk = pq + 4u * (uint32_t)k;
                            // (line 0 may begin before the half: a wrapped value is above it -- and then dword k may be the half's first
                            // occurrence although an earlier dword of the line equals it: line 0 takes no shortcut)
                            if ((pk - wbase < hlen) & (!dup[k] | (v == 0u) | (sh_inv != 0u))) // (inside the half; a history half keeps the LATEST: no shortcut)
                                (void)__hip_atomic_fetch_min(&shr[((g4[k] * 2654435761u) >> sh_shift) + sh_off], sh_base | (pk ^ sh_inv), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_WORKGROUP);
                        }
                    }
                }
            }
            uint4* tv = reinterpret_cast<uint4*>(tab);
            const uint4 e = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (uint32_t v = 0; v < (TAB * 2 / 16 + 63) / 64; ++v)
                if (v * 64 + lane < TAB * 2 / 16)
                    tv[v * 64 + lane] = e;
            if (tid == 0)
                flag[1] = gridDim.x + atomicAdd(worklist + 2u * ngroups + 1u, 1u);
        }
        __syncthreads();
        K5P(0);
        next_idx = flag[1];
        K5P(1);
        // ---- my unit, positions relative to the window ----
        const uint32_t my_start = (uint32_t)wave * sub_bytes;
        const bool have_unit = wih * sub_bytes < hlen && !(hist && hsel == 0u); // (a history half is staged and seeded, not parsed)
        const uint32_t my_len = have_unit ? (hlen - wih * sub_bytes < sub_bytes ? hlen - wih * sub_bytes : sub_bytes) : 0u;
        const uint32_t unit = blk.seg_base + gi * (uint32_t)G + hh * (uint32_t)(G / 2) + wih;
        const int64_t blk_left = (int64_t)blk.size - (int64_t)half_start - (int64_t)(wih * sub_bytes); // unit start .. block end
        int64_t sl = (int64_t)my_len - 4;
        if (sl > blk_left - 12)
            sl = blk_left - 12;
        const int32_t start_limit = have_unit ? (int32_t)((int64_t)my_start + sl) : -1;
        const int64_t el = (int64_t)my_len < blk_left - 5 ? (int64_t)my_len : (blk_left - 5 > 0 ? blk_left - 5 : 0);
        const uint32_t end_limit = my_start + (uint32_t)el;
        uint8_t* out = streams + (uint64_t)unit * (FMT == 1 ? sub_bytes : lz4_stream_stride(sub_bytes));
        uint64_t* recs = FMT == 1 ? zrecs + (uint64_t)unit * (sub_bytes >> 2) : nullptr;
        Lz4Seq st;
        st.op = 0;
        st.nseq = 0;
        st.anchor = my_start;
        st.first_lit = st.first_hdr = 0;
        st.have_first = false;
        // the private table starts with the aligned dwords of the unit before mine (my half's, or -- linked -- the other half's last)
        if (have_unit && (wih > 0u || (hsel && linked)) && !(dbg & 1u))
        {
            const uint32_t p0 = my_start - sub_bytes;
            const uint32_t l0 = (p0 + head) >> 4, l1 = (my_start + head + 15u) >> 4;
            for (uint32_t j0 = l0; j0 < l1; j0 += 256)
            {
                uint4 w[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                {
                    const uint32_t j = j0 + (uint32_t)u * 64u + (uint32_t)lane;
                    const uint32_t* q = sdata + lds_pidx(4u * j);
                    w[u] = j < l1 ? make_uint4(q[0], q[1], q[2], q[3]) : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                {
                    const uint32_t j = j0 + (uint32_t)u * 64u + (uint32_t)lane;
                    const uint32_t q = 16u * j - head;
                    const uint32_t g4[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                    {
                        const uint32_t pk = q + 4u * (uint32_t)k;
                        if (j < l1 && pk >= p0 && pk < my_start)
                            tab[lz4_tab_slot<TAB>(g4[k] * 2654435761u)] = (uint16_t)pk;
                    }
                }
            }
        }
        if (have_unit)
        {
            K5P(2);
            lz4_lane_parse2<TAB, FMT, SH>(sdata, head, tab, shr, sh_base, lane, my_start, my_len, start_limit, end_limit, sub_bytes >> 6, out, recs, st,
                                          dbg K5P_PASS, lo_bound, sh_shift, sh_off, linked ? 0xFFFFFFFFu : wbase, far1, far2, hist ? half_bytes : 0u, far3);
        }
        if constexpr (FMT == 1)
        {
            const uint32_t tail = have_unit ? my_start + my_len - st.anchor : 0u;
            if (st.nseq != 0u)
            {
                for (uint32_t j = lane; j < tail; j += 64)
                    out[st.op + j] = (uint8_t)lds_byte<PAD>(sdata, st.anchor + j + head);
            }
            else if (have_unit && spec_dst)
            {
                const uint32_t pos = half_start + wih * sub_bytes;
                const uint64_t o = 13u + (uint64_t)(pos / Z_PIECE) * (Z_PIECE + 3u) + 3u + pos % Z_PIECE;
                if (o + my_len <= (uint64_t)blk.dst_cap)
                    wave_copy_lds_to_global<PAD>(spec_dst + blk.dst_off + o, sdata, my_start + head, my_len, lane);
            }
            uint32_t uniform = 0;
            if (have_unit)
            {
                const uint32_t b0 = lds_byte<PAD>(sdata, my_start + head);
                const uint32_t rep = b0 * 0x01010101u;
                uint32_t diff = 0;
                if (64u * (uint32_t)lane + 4u <= my_len)
                    diff = lds_read32x<PAD>(sdata, my_start + 64u * (uint32_t)lane + head) ^ rep;
                if (__builtin_amdgcn_ballot_w64(diff != 0u) == 0ull)
#pragma unroll 4
                    for (uint32_t j = 0; j < 16u; ++j)
                    {
                        const uint32_t o = 64u * (uint32_t)lane + 4u * j;
                        if (o + 4u <= my_len)
                            diff |= lds_read32x<PAD>(sdata, my_start + o + head) ^ rep;
                        else if (o < my_len)
                            for (uint32_t k = o; k < my_len; ++k)
                                diff |= lds_byte<PAD>(sdata, my_start + k + head) ^ b0;
                    }
                uniform = __builtin_amdgcn_ballot_w64(diff != 0u) == 0ull ? (0x100u | b0) : 0u;
            }
            if (have_unit && lane == 0)
                reinterpret_cast<uint4*>(meta)[unit] = make_uint4(st.nseq, st.op + tail, tail, uniform);
        }
        else
        {
            if (spec_dst && have_unit && !st.have_first)
            {
                const uint64_t o = (uint64_t)(1u + lz4_len_bytes(blk.size)) + half_start + wih * sub_bytes;
                if (o + my_len <= (uint64_t)blk.dst_cap)
                    wave_copy_lds_to_global<PAD>(spec_dst + blk.dst_off + o, sdata, my_start + head, my_len, lane);
            }
            if (have_unit && lane == 0)
            {
                Lz4Meta m;
                m.seq_bytes = st.op;
                m.tail_lits = my_start + my_len - st.anchor;
                m.first_lit_len = st.first_lit;
                m.first_hdr_bytes = st.first_hdr;
                meta[unit] = m;
                if (st.op != 0u) // (the block's count of units with a sequence: k_lz4.hip, lz4_seq_units)
                    (void)__hip_atomic_fetch_add(lz4_seq_units(worklist, blk.grp_base), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        K5P(8);
        __syncthreads(); // every wave is done with the window before the next item overwrites it
        K5P(9);
    }
    K5P_FLUSH;
}

