// lz4_classify.inc -- part of k_lz4.hip (one translation unit; included there, inside its anonymous namespace, in this order):
// K5 pass 1, k_lz4_segments: the batch parser / the classification pass that skims incompressible groups and notes redundant ones
// TAB = entries of a wave's private table (any multiple of 8: the index is mulhi(hash, TAB), not a mask); G = units per window
// group = waves per workgroup: the batch parser, 8 x 4 KiB units per 32 KiB window group, THREE workgroups per CU.
// CLS = classification pass of the two-pass scheme: groups without redundancy are skimmed here and now (the fast geometry: 24 waves
// per CU), groups with redundancy are only NOTED -- the 16-unit group they belong to goes onto `worklist` -- and left to the lane
// parser (k_lz4_lanes2), which then runs over that list.  CLS 0 = the batch parser for everything: unit sizes other than 4 KiB.
template <int G, int TAB, int FMT, int CLS = 0>
__global__ __launch_bounds__(64 * G, 6) void k_lz4_segments(const uint8_t* __restrict__ src, const Lz4Block* __restrict__ blocks,
                                                             uint32_t nblocks, uint32_t grid2d, uint32_t sub_bytes,
                                                             uint8_t* __restrict__ streams, Lz4Meta* __restrict__ meta,
                                                             uint64_t* __restrict__ zrecs, uint8_t* __restrict__ spec_dst, uint32_t dbg,
                                                             uint64_t* __restrict__ lane_recs, uint32_t ngroups, uint32_t* __restrict__ worklist)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    constexpr bool PAD = false; // (the padded window is the lane parser's)
    const uint32_t data_bytes = lz4_window_lds_bytes(G * sub_bytes + 64u, PAD);
    uint32_t* sdata = smem;
    const uint8_t* sbytes = reinterpret_cast<const uint8_t*>(sdata);
    uint32_t* flag = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(smem) + data_bytes); // 16 bytes
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    uint16_t* tab = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(smem) + data_bytes + 16u) + (size_t)wave * TAB;
    K5P_DECL
    // one window group per workgroup
    {
    // Which block, which of its groups?  Two grids (lz4_grid_rule.h): two-dimensional -- blockIdx.y is the block, blockIdx.x the group
    // inside it, nothing to look up -- or one-dimensional over the batch's groups, the block found by bisection: ten dependent loads at
    // 900 blocks before the first data load, in a workgroup that lives for one group.
    uint32_t lo = blockIdx.y, gi = blockIdx.x;
    if (!grid2d)
    {
        uint32_t hi = nblocks;
        lo = 0;
        while (hi - lo > 1)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if ((CLS ? blocks[mid].cgrp_base : blocks[mid].grp_base) <= gi)
                lo = mid;
            else
                hi = mid;
        }
    }
    const Lz4Block blk = blocks[lo];
    if (!grid2d)
        gi -= CLS ? blk.cgrp_base : blk.grp_base;
    // (the two-dimensional grid is as wide as the longest block: beyond my block's groups there is nothing.  Wave-uniform, before any
    // LDS access and any barrier.)
    if (gi >= (CLS ? blk.ncgrp : blk.ngrp))
        return;
    const uint32_t group_start = gi * G * sub_bytes;                                   // block relative
    const uint32_t glen = blk.size - group_start < G * sub_bytes ? blk.size - group_start : G * sub_bytes;
    const uint8_t* g = src + blk.src_off + group_start;

    // ---- stage the whole group with every wave (16-byte loads from the aligned-down address), clear my table ----
    const uint32_t head_src = (uint32_t)((uintptr_t)g & 15u);
    // LDS byte address of position 0 of the group: the source's misalignment (the window is staged in aligned 16-byte lines)
    const uint32_t head = head_src;
    {
        const uint4* gv = reinterpret_cast<const uint4*>(g - head_src);
        const uint32_t nvec = (head_src + glen + 15u) >> 4;
        uint4* sv = reinterpret_cast<uint4*>(sdata);
        for (uint32_t v0 = 0; v0 < nvec; v0 += 64 * G * 4)
        {
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
            {
                const uint32_t v = v0 + u * 64 * G + tid;
                q[u] = v < nvec ? gv[v] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
            {
                const uint32_t v = v0 + u * 64 * G + tid;
                if (v < nvec)
                    sv[v] = q[u];
            }
        }
        uint4* tv = reinterpret_cast<uint4*>(tab);
        const uint32_t e1 = 0xFFFFFFFFu;
        const uint4 e = make_uint4(e1, e1, e1, e1);
#pragma unroll
        for (uint32_t v = 0; v < (TAB * 2 / 16 + 63) / 64; ++v) // TAB * 2 bytes, 64 lanes x 16 bytes per step
            if (v * 64 + lane < TAB * 2 / 16)
                tv[v * 64 + lane] = e;
        if (tid == 0)
            *flag = 0u;
    }
    __syncthreads();
    K5P(0);

    K5P(1);
    // ---- my unit, positions relative to the group start ----
    const uint32_t my_start = (uint32_t)wave * sub_bytes;
    const bool have_unit = my_start < glen;
    const bool emit_unit = have_unit;
    const uint32_t my_len = have_unit ? (glen - my_start < sub_bytes ? glen - my_start : sub_bytes) : 0u;
    const uint32_t unit = blk.seg_base + gi * G + (uint32_t)wave;
    // parsing limits (lz4.c:963-964: mflimit / matchlimit, applied at the BLOCK end)
    const int64_t blk_left = (int64_t)blk.size - (int64_t)group_start - (int64_t)my_start; // unit start .. block end
    int64_t sl = (int64_t)my_len - 4;
    if (sl > blk_left - 12)
        sl = blk_left - 12;
    const int32_t start_limit = have_unit ? (int32_t)((int64_t)my_start + sl) : -1; // < my_start when nothing may start
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
    uint32_t pos = my_start, nfail = 0;
    bool met = false; // the group rendezvous happens exactly once per wave
    uint32_t batches = 0;
    uint32_t pb0 = 0, pb1 = 0, pb2 = 0, pb3 = 0, ps0 = 1, ps1 = 1, ps2 = 1, ps3 = 1; // the probe batches (SGPRs)
    static_assert(LZ4_PROBE_BATCHES == 4, "probe bookkeeping is unrolled by hand");

    for (;;)
    {
        const bool more = have_unit && (int32_t)pos <= start_limit;
        // ---- after PROBE batches (or at the end of a short unit): does anybody in the group see redundancy? ----
        if (!met && (batches == LZ4_PROBE_BATCHES || !more))
        {
            if (st.have_first && lane == 0)
                *flag = 1u; // benign race: every writer stores the same value
            __syncthreads();
            if constexpr (CLS != 0)
            {
                if (*flag != 0u)
                {
                    // redundancy: this group is the lane parser's.  Note the 16-unit group it belongs to (once) and leave.
                    if (tid == 0)
                    {
                        const uint32_t g16 = blk.grp_base + gi / (uint32_t)(LZ4_G_LANES / LZ4_G_BATCH);
                        // (bit h of the group's word: its half h holds redundancy; a half WITHOUT it is skimmed by this pass, and the
                        // lane kernel only takes its bytes as history)
                        // one atomic nobody waits for: k_lz4_pair_halves reads the groups' words.  (Round 5: the list of noted groups
                        // that this thread used to build -- an atomic OR whose answer decides about an atomic add whose answer is the
                        // slot -- kept a workgroup that had nothing left to do on its CU for two round trips to memory.)
                        (void)__hip_atomic_fetch_or(&worklist[1u + ngroups + g16], 1u << (gi & 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    return;
                }
            }
            if (*flag != 0u && wave != 0 && have_unit && !(dbg & 1u))
            {
                // learn the history: insert every position before my unit, oldest first (plain stores, four
                // independent positions per lane in flight), then re-insert my own probed positions on top
                // every 4th position is enough: a match found one to three bytes late is recovered by the
                // backward extension, and the small table is polluted less (CPU model of this parse: ratio 1.755 -> 1.785)
                for (uint32_t q0 = 0; q0 < my_start; q0 += 1024) // my_start is a multiple of 1024
                {
                    uint32_t hv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        hv[u] = __umulhi(lds_read32(sdata, q0 + 4u * (u * 64 + (uint32_t)lane) + head) * 2654435761u, (uint32_t)TAB);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        tab[hv[u]] = (uint16_t)(q0 + 4u * (u * 64 + (uint32_t)lane));
                }
#define LT_REPLAY(r, PB, PS)                                                                            \
    if ((r) < batches)                                                                                  \
    {                                                                                                   \
        const uint32_t rp = (PB) + (uint32_t)lane * (PS);                                               \
        if ((int32_t)rp <= start_limit)                                                                 \
            tab[__umulhi(lds_read32(sdata, rp + head) * 2654435761u, (uint32_t)TAB)] = (uint16_t)rp;         \
    }
                LT_REPLAY(0u, pb0, ps0)
                LT_REPLAY(1u, pb1, ps1)
                LT_REPLAY(2u, pb2, ps2)
                LT_REPLAY(3u, pb3, ps3)
#undef LT_REPLAY
            }
            else if (*flag == 0u && more && !(dbg & 16u))
                nfail += 24u; // nobody in the 32 KiB group matched anything in its probe batches: one twin round skims the rest
            met = true;
        }
        if (!more)
            break;
        if (batches == 0) { pb0 = pos; ps0 = 1u + nfail; }
        else if (batches == 1) { pb1 = pos; ps1 = 1u + nfail; }
        else if (batches == 2) { pb2 = pos; ps2 = 1u + nfail; }
        else if (batches == 3) { pb3 = pos; ps3 = 1u + nfail; }
        ++batches;

        // ---- probe 64 positions (stride grows with consecutive misses, lz4.c:1044-1053) ----
        uint32_t stride = 1u + nfail;
        uint32_t p = pos + (uint32_t)lane * stride;
        bool valid = (int32_t)p <= start_limit;
        uint32_t v = 0, cand = LZ4_EMPTY, h = 0;
        bool ok = false;
        if (met && nfail != 0u && !(dbg & 8u))
        {
            // Miss mode: the NEXT batch is probed in the same breath (its LDS round trips overlap this batch's): a
            // unit of incompressible data is a chain of dependent probes and nothing else, so this halves its
            // latency.  The second batch reads the table before the first one's inserts and is only inserted if the
            // first one missed.
            const uint32_t pos2 = pos + 64u * stride;
            const uint32_t p2 = pos2 + (uint32_t)lane * (stride + 1u);
            const bool valid2 = (int32_t)p2 <= start_limit;
            uint32_t v2 = 0, cand2 = LZ4_EMPTY, h2 = 0;
            if (valid)
            {
                v = lds_read32(sdata, p + head);
                h = __umulhi(v * 2654435761u, (uint32_t)TAB);
                cand = tab[h];
            }
            if (valid2)
            {
                v2 = lds_read32(sdata, p2 + head);
                h2 = __umulhi(v2 * 2654435761u, (uint32_t)TAB);
                cand2 = tab[h2];
            }
            if (valid)
                tab[h] = (uint16_t)p;
            bool ok2 = false;
            if (valid && cand != LZ4_EMPTY && cand < p)
                ok = lds_read32(sdata, cand + head) == v;
            if (valid2 && cand2 != LZ4_EMPTY && cand2 < p2)
                ok2 = lds_read32(sdata, cand2 + head) == v2;
            if (__builtin_amdgcn_ballot_w64(ok) == 0ull)
            {
                if (valid2)
                    tab[h2] = (uint16_t)p2;
                if (__builtin_amdgcn_ballot_w64(ok2) == 0ull)
                {
                    pos = pos2 + 64u * (stride + 1u);
                    nfail += 2u;
                    continue;
                }
                pos = pos2; // the second batch becomes the current one
                ++nfail;
                stride += 1u;
                p = p2;
                cand = cand2;
                ok = ok2;
            }
        }
        else
        {
            if (valid)
            {
                v = lds_read32(sdata, p + head);
                h = __umulhi(v * 2654435761u, (uint32_t)TAB);
                cand = tab[h];
            }
            // every lane has read the table before anyone updates it (same wave: LDS operations execute in order)
            if (valid)
                tab[h] = (uint16_t)p;
            if (valid && cand != LZ4_EMPTY && cand < p)
                ok = lds_read32(sdata, cand + head) == v;
        }
        // matches whose source lies in the same batch are invisible to the table: look 1, 2, 4, 8 lanes back
        if (nfail == 0 && !(dbg & 2u))
        {
            uint32_t best = 0;
            bool found = false;
            // the four exchanges are issued together (one LDS round trip instead of four); a valid lane's lower neighbours
            // are valid too (their positions are smaller), so their validity needs no exchange
            uint32_t ovs[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                ovs[t] = __shfl_up(v, 8 >> t, 64);
#pragma unroll
            for (int t = 0; t < 4; ++t) // smallest distance wins (assigned last)
            {
                const int d = 8 >> t;
                if (valid && lane >= d && ovs[t] == v)
                {
                    best = p - (uint32_t)d * stride;
                    found = true;
                }
            }
            if (found && (!ok || best > cand))
            {
                cand = best;
                ok = true;
            }
        }
        uint64_t hits = __builtin_amdgcn_ballot_w64(ok);
        if (hits == 0ull)
        {
            pos += 64u * stride;
            ++nfail;
            continue;
        }
        if constexpr (CLS != 0)
        {
            if (!met)
            {
                // classification pass: one hit settles it -- the group is the lane parser's.  Raise the flag and go to the rendezvous
                // without parsing anything.  (The other waves are NOT polled out of their probe batches: a flag read per batch is one
                // more dependent LDS round trip in the chain that incompressible data consists of -- measured +8 % on random data.)
                st.have_first = true;
                if (lane == 0)
                    *flag = 1u;
                pos = (uint32_t)(start_limit + 1);
                continue;
            }
        }
        if (dbg & 4u)
        {
            // ablation: every hit at or after the previous match handled cooperatively with full extension
            do
            {
                const int f = __builtin_ctzll(hits);
                hits &= hits - 1ull;
                const uint32_t pf = pos + (uint32_t)f * stride;
                if (pf < st.anchor)
                    continue;
                lz4_coop_sequence<FMT>(sbytes, head, out, recs, lane, end_limit, pf, __builtin_amdgcn_readlane(cand, f), 4u, true, true, st);
            } while (hits);
            const uint32_t np = pos + 64u * stride;
            pos = np > st.anchor ? np : st.anchor;
            nfail = 0;
            continue;
        }
        if (stride != 1u)
        {
            // sparse mode (after misses): only the first hit, handled by the whole wave
            const int f = __builtin_ctzll(hits);
            lz4_coop_sequence<FMT>(sbytes, head, out, recs, lane, end_limit, pos + (uint32_t)f * stride, __builtin_amdgcn_readlane(cand, f), 4u,
                              true, true, st);
            pos = st.anchor;
            nfail = 0;
            continue;
        }
        // ---- dense mode: every lane measures its own match, in parallel: 16 bytes per LDS round trip (four dword pairs
        // in flight at once -- the batch is a latency chain, not a bandwidth problem), at most 36 bytes ----
        uint32_t mlen = ok ? 4u : 0u;
        bool act = ok;
        const uint32_t maxlen = ok ? end_limit - p : 0u;
#pragma unroll 1
        for (int t = 0; t < 2; ++t)
        {
            if (__builtin_amdgcn_ballot_w64(act) == 0ull)
                break;
            if (act)
            {
                const uint32_t a0 = p + mlen + head, b0 = cand + mlen + head;
                const uint32_t x0 = lds_read32(sdata, a0) ^ lds_read32(sdata, b0);
                const uint32_t x1 = lds_read32(sdata, a0 + 4u) ^ lds_read32(sdata, b0 + 4u);
                const uint32_t x2 = lds_read32(sdata, a0 + 8u) ^ lds_read32(sdata, b0 + 8u);
                const uint32_t x3 = lds_read32(sdata, a0 + 12u) ^ lds_read32(sdata, b0 + 12u);
                uint32_t add = 16u;
                if (x0)
                    add = (uint32_t)__builtin_ctz(x0) >> 3;
                else if (x1)
                    add = 4u + ((uint32_t)__builtin_ctz(x1) >> 3);
                else if (x2)
                    add = 8u + ((uint32_t)__builtin_ctz(x2) >> 3);
                else if (x3)
                    add = 12u + ((uint32_t)__builtin_ctz(x3) >> 3);
                mlen += add;
                if (add != 16u)
                    act = false;
                if (mlen >= maxlen)
                {
                    mlen = maxlen;
                    act = false;
                }
            }
        }
        const uint64_t longs = __builtin_amdgcn_ballot_w64(act); // still equal after 36 bytes: extend when selected
        // ... and how far it could grow backwards (at most 8 bytes, both dword pairs read at once; the anchor bounds it
        // at selection)
        uint32_t nbk = 0;
        if (ok && cand >= 8u)
        {
            const uint32_t x = lds_read32(sdata, p - 4u + head) ^ lds_read32(sdata, cand - 4u + head);
            const uint32_t y = lds_read32(sdata, p - 8u + head) ^ lds_read32(sdata, cand - 8u + head);
            nbk = x ? (uint32_t)__builtin_clz(x) >> 3 : (y ? 4u + ((uint32_t)__builtin_clz(y) >> 3) : 8u);
        }
        // ---- greedy selection in position order: a scalar walk over the SELECTED hits only ----
        uint64_t rem = hits, vecsel = 0ull;
        uint32_t sel_v = 0; // selected lanes: output offset << 8 | backward bytes << 4 | literal count
        while (rem)
        {
            if (st.anchor > pos)
            {
                const uint32_t sh = st.anchor - pos; // lanes whose position is already covered
                rem = sh >= 64u ? 0ull : rem & (~0ull << sh);
                if (!rem)
                    break;
            }
            const int f = __builtin_ctzll(rem);
            rem &= rem - 1ull;
            const uint32_t pf = pos + (uint32_t)f;
            const bool isl = (longs >> f) & 1ull;
            const uint32_t room = pf - st.anchor;
            if (isl || room > 20u)
            {
                lz4_coop_sequence<FMT>(sbytes, head, out, recs, lane, end_limit, pf, __builtin_amdgcn_readlane(cand, f),
                                  __builtin_amdgcn_readlane(mlen, f), isl, true, st);
                continue;
            }
            uint32_t nb = __builtin_amdgcn_readlane(nbk, f);
            nb = nb < room ? nb : room;
            const uint32_t lit = room - nb;
            const uint32_t len = __builtin_amdgcn_readlane(mlen, f) + nb;
            if (lit > 12u)
            {
                lz4_coop_sequence<FMT>(sbytes, head, out, recs, lane, end_limit, pf - nb, __builtin_amdgcn_readlane(cand, f) - nb, len, false,
                                  false, st);
                continue;
            }
            // short literals, match <= 44 bytes: emitted below by the lane itself
            sel_v = lane == f ? (FMT == 1 ? st.nseq << 20 : 0u) | (st.op << 8) | (nb << 4) | lit : sel_v;
            vecsel |= 1ull << f;
            if (!st.have_first)
            {
                st.have_first = true;
                st.first_lit = lit;
                st.first_hdr = 1u;
            }
            if constexpr (FMT == 1)
            {
                st.op += lit;
                st.nseq += 1u;
            }
            else
                st.op += lit + 3u + (len - 4u >= 15u ? 1u : 0u);
            st.anchor = pf + len - nb;
        }
        if ((vecsel >> lane) & 1ull)
        {
            const uint32_t lit = sel_v & 15u;
            const uint32_t nb = (sel_v >> 4) & 15u;
            const uint32_t lit_start_v = p - nb - lit;
            const uint32_t off = p - cand;
            if constexpr (FMT == 1)
            {
                uint8_t* o = out + ((sel_v >> 8) & 0xFFFu);
                for (uint32_t j = 0; j < lit; ++j)
                    o[j] = sbytes[lit_start_v + j + head];
                recs[sel_v >> 20] = (uint64_t)lit | ((uint64_t)(mlen + nb) << 16) | ((uint64_t)off << 32);
            }
            else
            {
                const uint32_t mcode = mlen + nb - 4u; // <= 40: at most one length byte
                uint8_t* o = out + (sel_v >> 8);
                o[0] = (uint8_t)((lit << 4) | (mcode < 15u ? mcode : 15u));
                for (uint32_t j = 0; j < lit; ++j)
                    o[1u + j] = sbytes[lit_start_v + j + head];
                o[1u + lit] = (uint8_t)off;
                o[2u + lit] = (uint8_t)(off >> 8);
                if (mcode >= 15u)
                    o[3u + lit] = (uint8_t)(mcode - 15u);
            }
        }
        const uint32_t np = pos + 64u;
        pos = np > st.anchor ? np : st.anchor;
        nfail = 0;
    }
    if constexpr (FMT == 1)
    {
        // the unit's trailing literals complete its literal buffer; meta = ZbUnitMeta {nseq, nlit, tail, 0}
        const uint32_t tail = emit_unit ? my_start + my_len - st.anchor : 0u;
        if (st.nseq != 0u)
        {
            for (uint32_t j = lane; j < tail; j += 64)
                out[st.op + j] = (uint8_t)lds_byte<PAD>(sdata, st.anchor + j + head);
        }
        else if (emit_unit && spec_dst)
        {
            // A unit without a sequence has no literal buffer (the entropy stage reads its bytes from the source,
            // ZbInput.src).  If its whole 128 KiB piece is like that the piece will most likely be a Raw_Block, and if the
            // pieces before it are raw too its bytes belong at  frame header + pieces * (3 + 128 KiB) + 3 + offset: put
            // them there now, from LDS; k_zstd_emit then only writes the 3-byte block header (and copies as usual when
            // the guess was wrong).
            const uint32_t pos = group_start + my_start;
            const uint64_t o = 13u + (uint64_t)(pos / Z_PIECE) * (Z_PIECE + 3u) + 3u + pos % Z_PIECE;
            if (o + my_len <= (uint64_t)blk.dst_cap)
                wave_copy_lds_to_global<PAD>(spec_dst + blk.dst_off + o, sdata, my_start + head, my_len, lane);
        }
        // is the unit one repeated byte?  (zstd stores a 128 KiB piece made of such units as an RLE_Block)
        uint32_t uniform = 0;
        if (emit_unit)
        {
            const uint32_t b0 = lds_byte<PAD>(sdata, my_start + head);
            const uint32_t rep = b0 * 0x01010101u;
            uint32_t diff = 0;
            // almost always settled by the first dword of every lane's 64 bytes
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
        if (emit_unit && lane == 0)
            reinterpret_cast<uint4*>(meta)[unit] = make_uint4(st.nseq, st.op + tail, tail, uniform);
    }
    else
    {
    // A unit without a single match is all literals.  If that turns out to be true of the WHOLE block (incompressible
    // data -- the common case for already-compressed assets), the payload is one literal run: header, then the source
    // bytes, and this unit's bytes belong at  header + its offset in the block.  They are still in LDS, so they are put
    // there now, speculatively; the stitch then only writes the header for such blocks instead of reading and writing
    // them again (a block that does have matches is laid out by the stitch as usual, overwriting these bytes).
    if (FMT == 0 && spec_dst && emit_unit && !st.have_first)
    {
        const uint64_t o = (uint64_t)(1u + lz4_len_bytes(blk.size)) + group_start + my_start;
        if (o + my_len <= (uint64_t)blk.dst_cap)
            wave_copy_lds_to_global<PAD>(spec_dst + blk.dst_off + o, sdata, my_start + head, my_len, lane);
    }
    if (emit_unit && lane == 0)
    {
        Lz4Meta m;
        m.seq_bytes = st.op;
        m.tail_lits = my_start + my_len - st.anchor;
        m.first_lit_len = st.first_lit;
        m.first_hdr_bytes = st.first_hdr;
        meta[unit] = m;
        // the block's count of units with a sequence (lz4_seq_units): k_lz4_stitch_scan walks only blocks that have one.  One
        // relaxed atomic nobody waits for, none on incompressible data.
        if (CLS != 0 && st.op != 0u)
            (void)__hip_atomic_fetch_add(lz4_seq_units(worklist, blk.grp_base), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    } // FMT 0
    K5P(8);
    K5P(9);
    } // the group
}
