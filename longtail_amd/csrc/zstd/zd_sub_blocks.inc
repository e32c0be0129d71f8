// zd_sub_blocks.inc -- part of k_zstd_decode.hip (one translation unit; included there, inside its anonymous namespace, in this order):
// this library's own frames: pieces that are runs of sub-blocks -- k_zstd_sub_entropy (streams per lane)
// ---------------------------------------------------------------------------------------------------
// Pieces that are runs of SUB-BLOCKS (kind 3): k_zstd_sub_entropy + k_zstd_execute<true>.
// One wave per piece.  Lane u owns unit u's block: it finds it through the frame's directory, checks the Block_Header against the
// directory, parses the literals and sequences section headers.  The Huffman tree and the three FSE tables come with the first
// block that needs them (everything else is treeless / Predefined or Repeat_Mode) and are built once, by the decoder core's
// own readers.  Then every lane decodes streams of its own: the up to 128 Huffman streams of the piece's literals (into the piece's
// literal buffer, back to back in block order), and the up to 32 sequence bit-streams (lane u the sequences of block u, as records
// {literal length, match length, offset value} into the piece's record array).  A block's literals after its last sequence join
// the literal length of the next sequence of the piece, so what k_zstd_execute<true> sees is ONE run of sequences over ONE run of
// literals, exactly what it executes for a one-block piece.
// STRICT like the one-block piece decoder: a block may not use repeat offsets; more than that, anything that is not what
// zb_encode_piece_sub writes (a second tree, tables sent twice, a block that does not regenerate exactly its unit, a header that
// disagrees with the directory) sends the whole payload to the serial decoder (retry[payload]), which accepts and rejects what it
// always did.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t zs_bits(const uint8_t* base, uint32_t bitpos, uint32_t n) // bits [bitpos, bitpos + n), n <= 32
{
    const uint32_t b1 = (bitpos + n + 7u) >> 3; // the 8 bytes that END with the byte holding the field's top bit: never past the stream
    uint64_t w;
    __builtin_memcpy(&w, base + (int64_t)b1 - 8, 8);
    return (uint32_t)(w >> (bitpos + 64u - 8u * b1)) & (uint32_t)((1ull << n) - 1ull);
}

// A lane's backward bit reader with the stream ahead of it in registers: 128 bits [top - 128, top) plus the 64 below them already
// on their way, so that no load sits on the chain state -> bits -> next state (one 8-byte load per 64 bits consumed, issued a
// window ahead).  Loads may reach up to 24 bytes below the stream: `reach` = how many bytes below it are readable (what lies
// there is never used).
struct ZsWin
{
    const uint8_t* base;
    uint64_t hi, lo, nx;
    int32_t top;   // bit index (relative to base) one past the window
    int32_t reach; // lowest readable byte offset relative to base (<= 0)
    __device__ __forceinline__ uint64_t load(int32_t byte_off) const
    {
        uint64_t w;
        const int32_t o = byte_off < reach ? reach : byte_off;
        __builtin_memcpy(&w, base + o, 8);
        return w;
    }
    __device__ __forceinline__ void open(const uint8_t* b, uint32_t size, uint32_t below)
    {
        base = b;
        reach = -(int32_t)below;
        top = (int32_t)(8u * size);
        hi = load((int32_t)size - 8);
        lo = load((int32_t)size - 16);
        nx = load((int32_t)size - 24);
    }
    // make bits [pos - need, pos) part of the window (need <= 64; pos <= top)
    __device__ __forceinline__ void ensure(uint32_t pos, uint32_t need)
    {
        if ((int32_t)pos - (int32_t)need < top - 128)
        {
            hi = lo;
            lo = nx;
            top -= 64;
            nx = load((top >> 3) - 24);
        }
    }
    __device__ __forceinline__ uint64_t get64(uint32_t bitpos) const // bits [bitpos, bitpos + 64) (zeros above the window's top)
    {
        const uint32_t s = (uint32_t)((int32_t)bitpos - (top - 128)); // 0 .. 127
        return s >= 64u ? hi >> (s - 64u) : (s ? (lo >> s) | (hi << (64u - s)) : lo);
    }
    // the 64 bits below `pos`, the next bit to read on top (fewer than 64 bits left: zeros below them)
    __device__ __forceinline__ uint64_t below(uint32_t pos) const
    {
        return pos >= 64u ? get64(pos - 64u) : (pos ? get64(0u) << (64u - pos) : 0ull);
    }
    __device__ __forceinline__ uint32_t get(uint32_t bitpos, uint32_t n) const // bits [bitpos, bitpos + n), n <= 32, inside the window
    {
        const uint32_t s = (uint32_t)((int32_t)bitpos - (top - 128)); // 0 .. 127
        const uint64_t v = s >= 64u ? hi >> (s - 64u) : (s ? (lo >> s) | (hi << (64u - s)) : lo);
        return (uint32_t)v & (uint32_t)((1ull << n) - 1ull);
    }
};

// The sequence lanes: every lane with `act` decodes ONE bit-stream of nbseq sequences (tables packed in shared memory, one 8-byte
// entry per state) into records {literal length:20 | match length:20 | offset value:24}.  One loop for the wave, a lane takes part
// while its stream has sequences left (no lane leaves early: a lane that finds an error only stops decoding).  Per sequence: the
// three entries, ONE 64-bit view of the bits below the position (a second one only when offset + lengths + states exceed 64 bits),
// the fields shifted off its top.  STRICT: offset values 1..3 (repeat offsets) are errors; otherwise they stay in the record for
// whoever executes it in order.
// STRICT 0: offset values 1..3 stay in the record; 1: they are errors; 2: resolved with a block-local history (version-3 frames)
template <int STRICT>
__device__ __forceinline__ void zs_seq_lanes(bool act, const uint8_t* stream, uint32_t ssize, uint32_t below, uint32_t nbseq, uint32_t log_l,
                                             uint32_t log_o, uint32_t log_m, const uint64_t* pk_ll, const uint64_t* pk_of, const uint64_t* pk_ml,
                                             uint64_t* recs, bool& bad, uint32_t& sum_ll, uint32_t& sum_ml)
{
    uint32_t pos = 0, sl = 0, so = 0, sm = 0;
    [[maybe_unused]] uint32_t r1 = 0, r2 = 0, r3 = 0; // STRICT: the block's own offset history, 0 = unknown
    ZsWin w;
    w.base = stream;
    w.hi = w.lo = w.nx = 0;
    w.top = 0;
    w.reach = 0;
    if (act)
    {
        if (ssize == 0u || stream[ssize - 1u] == 0u)
            bad = true;
        else
        {
            pos = (ssize - 1u) * 8u + (31u - (uint32_t)__builtin_clz((uint32_t)stream[ssize - 1u]));
            w.open(stream, ssize, below);
            if (log_l + log_o + log_m > pos)
                bad = true;
            else
            {
                pos -= log_l;
                sl = w.get(pos, log_l);
                pos -= log_o;
                so = w.get(pos, log_o);
                pos -= log_m;
                sm = w.get(pos, log_m);
            }
        }
        act = !bad;
    }
    const bool had = act;
    for (uint32_t k = 0; __builtin_amdgcn_ballot_w64(act && k < nbseq) != 0ull; ++k)
    {
        if (act && k < nbseq)
        {
            const uint64_t el = pk_ll[sl], eo = pk_of[so], em = pk_ml[sm];
            const uint32_t l0 = (uint32_t)el, o0 = (uint32_t)eo, m0 = (uint32_t)em;
            const uint32_t ob = o0 >> 24, mb = m0 >> 24, lb = l0 >> 24;
            const uint32_t nbl = (l0 >> 16) & 255u, nbm = (m0 >> 16) & 255u, nbo = (o0 >> 16) & 255u;
            const bool more = k + 1u < nbseq;
            const uint32_t n1 = ob + mb + lb, n2 = more ? nbl + nbm + nbo : 0u; // <= 63, <= 26
            if (n1 + n2 > pos)
            {
                bad = true;
                act = false;
            }
            else
            {
                w.ensure(pos, 64u);
                uint64_t acc = w.below(pos);
                const uint32_t ov = (uint32_t)(eo >> 32) + (uint32_t)((acc >> 1) >> (63u - ob));
                acc <<= ob;
                const uint32_t t2 = (uint32_t)((acc >> 1) >> (63u - (mb + lb))); // match-length and literal-length bits are adjacent
                acc <<= mb + lb;
                const uint32_t ml = (uint32_t)(em >> 32) + (t2 >> lb);
                const uint32_t ll = (uint32_t)(el >> 32) + (t2 & ((1u << lb) - 1u));
                if (n1 + n2 > 64u) // (rare: the view does not reach the state fields)
                {
                    w.ensure(pos - n1, 32u);
                    acc = w.below(pos - n1);
                }
                if (more)
                {
                    const uint32_t t3 = (uint32_t)((acc >> 1) >> (63u - n2)); // LL, ML, OF from the top
                    sl = (l0 & 0xFFFFu) + (t3 >> (nbm + nbo));
                    sm = (m0 & 0xFFFFu) + ((t3 >> nbo) & ((1u << nbm) - 1u));
                    so = (o0 & 0xFFFFu) + (t3 & ((1u << nbo) - 1u));
                }
                pos -= n1 + n2;
                uint32_t ovr = ov;
                if constexpr (STRICT == 1)
                {
                    if (ov <= 3u)
                        bad = true; // (a version-2 frame writes plain offsets only)
                }
                if constexpr (STRICT == 2)
                {
                    // Repeat offsets, resolved here: this library's encoder only refers to history entries that the block's own
                    // sequences have set (zb_encode_piece_sub, ZB_F_REPCODES), so the lane starts with an unknown history (0) and a
                    // code that would read an unknown entry is what "needs the block before" now means.
                    const uint32_t used = ov > 3u ? 0u : (ll != 0u ? ov : ov + 1u); // entry 1..3, 4 = entry 1 minus one, 0 = a new offset
                    uint32_t off = ov - 3u;
                    if (used)
                    {
                        off = used == 1u ? r1 : used == 2u ? r2 : used == 3u ? r3 : r1 - 1u;
                        if (off == 0u || (used == 4u && r1 == 0u))
                            bad = true;
                    }
                    if (used == 2u)
                    {
                        r2 = r1;
                        r1 = off;
                    }
                    else if (used != 1u)
                    {
                        r3 = r2;
                        r2 = r1;
                        r1 = off;
                    }
                    ovr = off + 3u;
                }
                if (ovr >= (1u << 24))
                    bad = true;
                sum_ll += ll;
                sum_ml += ml;
                recs[k] = (uint64_t)ll | ((uint64_t)ml << 20) | ((uint64_t)ovr << 40);
            }
        }
    }
    if (had && !bad && pos != 0u)
        bad = true; // the bit-stream must be consumed exactly
}

__global__ __launch_bounds__(64) void k_zstd_sub_entropy(const uint8_t* __restrict__ src, const ZBlock* __restrict__ blocks, const ZItem* __restrict__ items,
                                                         const uint32_t* __restrict__ item_count, uint32_t item0, uint32_t item1,
                                                         uint8_t* __restrict__ lit_scratch, uint64_t* __restrict__ rec_scratch,
                                                         ZPrep* __restrict__ prep, const uint32_t* __restrict__ out_sizes,
                                                         uint32_t* __restrict__ retry, uint32_t* __restrict__ ticket, const uint32_t* __restrict__ perm)
{
    __shared__ ZdShared sh;
    __shared__ uint4 s_streams[4 * ZB_MAX_UNITS]; // {source offset inside the piece, bytes, literal offset, symbols}
    __shared__ __attribute__((aligned(16))) uint8_t s_desc[512 + 256]; // the table descriptions and the tree description, staged: lane 0 parses
                                                                      // them bit by bit, and a byte from global memory costs it a round trip
    const uint32_t nitems = *item_count < item1 ? *item_count : item1;
    const int lane = threadIdx.x;
    uint64_t* const pk_ll = reinterpret_cast<uint64_t*>(sh.huf); // packed tables {base:16 | state bits:8 | extra bits:8 | baseline:32},
    uint64_t* const pk_ml = pk_ll + 512;                         // over the Huffman table (done with by then) ...
    uint64_t* const pk_of = reinterpret_cast<uint64_t*>(&sh.wtab); // ... and the weights' table
    static_assert(sizeof(sh.huf) >= 2 * 512 * 8 && sizeof(sh.wtab) >= 256 * 8, "room for the packed tables");
    for (;;)
    {
        // Pieces cost very different amounts (raw units next to units full of sequences): the persistent waves draw them from a
        // counter.  Every lane takes part in the draw (lane 0 adds one, the others zero; the compiler turns it into one atomic per
        // wave).  With "if (lane == 0) t = atomicAdd(..)" hipcc (ROCm 7.2) threaded such a loop: lane 0 and the other 63 lanes came
        // back to the loop head separately, the 63 with t = 0, and worked on ticket 0 a second time without lane 0 -- a hang.
        __builtin_amdgcn_wave_barrier();
        uint32_t t = atomicAdd(ticket, lane == 0 ? 1u : 0u);
        t = __builtin_amdgcn_readfirstlane(t);
        if (item0 + t >= nitems)
            break;
        const uint32_t i = perm[item0 + t]; // (link-major order: k_zstd_rows)
        const ZItem it = items[i];
        if (it.kind != 3u)
            continue;
        __syncthreads();
#ifdef LTHIP_ZB_PROF
        if (lane == 0)
            g_zb_last[blockIdx.x] = wall_clock64();
#endif
        const ZBlock blk = blocks[it.payload];
        const uint32_t slot = t;
        uint8_t* lits = lit_scratch + (uint64_t)slot * (ZD_LIT_MAX + 64u);
        uint64_t* recs = rec_scratch + (uint64_t)slot * ZREC_MAX;
        const uint8_t* p = src + it.src_off;
        const uint8_t* dir = src + blk.src_off + it.aux;
        const uint32_t content = out_sizes[it.payload] == ZD_ERROR ? 0u : out_sizes[it.payload];
        const uint32_t expect = content > it.out0 ? (content - it.out0 < ZB ? content - it.out0 : ZB) : 0u;
        const uint32_t nunits = (expect + ZB_UNIT - 1u) / ZB_UNIT;
        const bool mine = (uint32_t)lane < nunits;
        bool bad = expect == 0u;
        if (lane == 0)
        {
            sh.v[ZDV_ERR] = 0;
            sh.v[ZDV_PREP] = 0;
            sh.huf_valid = 0;
        }
        // ---- my block: where, what ----
        uint32_t e = 0;
        if (mine)
            e = (uint32_t)dir[2 * lane] | ((uint32_t)dir[2 * lane + 1] << 8);
        const uint32_t raw = e >> 15, csz = e & 0x7FFFu;
        uint32_t total;
        const uint32_t off = z_wave_scan_excl(mine ? 3u + csz : 0u, lane, &total);
        bad = bad || total != it.size;
        const uint32_t ubytes = mine ? ((uint32_t)lane + 1u == nunits ? expect - (uint32_t)lane * ZB_UNIT : ZB_UNIT) : 0u;
        const uint8_t* c = p + off + 3u; // my block's content
        uint32_t lmode = 0, nlit = 0, lhdr = 0, lcs = 0, nstr = 0, nbseq = 0, shdr = 0, modes = 0;
        if (mine && !bad)
        {
            const uint32_t h = (uint32_t)p[off] | ((uint32_t)p[off + 1u] << 8) | ((uint32_t)p[off + 2u] << 16);
            const uint32_t is_last = (it.out0 + expect == content && (uint32_t)lane + 1u == nunits) ? 1u : 0u;
            if ((h & 1u) != is_last || ((h >> 1) & 3u) != (raw ? 0u : 2u) || (h >> 3) != csz || (raw && csz != ubytes))
                bad = true;
            else if (raw)
                nlit = ubytes; // the unit's bytes are its literals
            else if (csz < 2u)
                bad = true;
            else
            {
                const uint32_t b0 = c[0], sf = (b0 >> 2) & 3u;
                lmode = b0 & 3u;
                if (lmode < 2u)
                {
                    lhdr = (sf & 1u) == 0u ? 1u : sf == 1u ? 2u : 3u;
                    if (lhdr > csz)
                        bad = true;
                    else
                    {
                        nlit = lhdr == 1u ? b0 >> 3 : lhdr == 2u ? ((uint32_t)c[0] | ((uint32_t)c[1] << 8)) >> 4
                                                                : ((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16)) >> 4;
                        lcs = lmode == 0u ? nlit : 1u;
                    }
                }
                else
                {
                    lhdr = sf < 2u ? 3u : sf == 2u ? 4u : 5u;
                    if (lhdr > csz)
                        bad = true;
                    else if (lhdr == 3u)
                    {
                        const uint32_t hh = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
                        nlit = (hh >> 4) & 0x3FFu;
                        lcs = hh >> 14;
                    }
                    else if (lhdr == 4u)
                    {
                        const uint32_t hh = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
                        nlit = (hh >> 4) & 0x3FFFu;
                        lcs = hh >> 18;
                    }
                    else
                    {
                        const uint32_t hh = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
                        nlit = (hh >> 4) & 0x3FFFFu;
                        lcs = (hh >> 22) | ((uint32_t)c[4] << 10);
                    }
                    nstr = sf == 0u ? 1u : 4u;
                }
                if (!bad && (nlit > ubytes || lcs >= csz - lhdr)) // (at least one byte of sequences section follows)
                    bad = true;
                if (!bad)
                {
                    const uint32_t sp = lhdr + lcs;
                    const uint32_t n0 = c[sp];
                    if (n0 == 0u)
                    {
                        shdr = 1;
                        bad = sp + 1u != csz;
                    }
                    else
                    {
                        if (n0 < 128u)
                        {
                            nbseq = n0;
                            shdr = 1;
                        }
                        else if (n0 < 255u)
                        {
                            bad = sp + 2u > csz;
                            nbseq = bad ? 0u : ((n0 - 128u) << 8) + c[sp + 1u];
                            shdr = 2;
                        }
                        else
                            bad = true; // 0x7F00 sequences and more: not in a 4 KiB unit
                        if (!bad && (sp + shdr + 1u >= csz || nbseq > ZB_UNIT_SEQ_MAX || nbseq == 0u))
                            bad = true;
                        if (!bad)
                        {
                            modes = c[sp + shdr];
                            shdr += 1u;
                            bad = (modes & 3u) != 0u;
                        }
                    }
                }
            }
        }
#ifdef LTHIP_ZB_PROF
        ZB_MARK(19);
#endif
        // ---- who brings the tree, who the tables; is everybody else consistent with them? ----
        const uint64_t treem = __builtin_amdgcn_ballot_w64(mine && !raw && lmode == 2u);
        const uint64_t lessm = __builtin_amdgcn_ballot_w64(mine && !raw && lmode == 3u);
        const uint64_t seqm = __builtin_amdgcn_ballot_w64(mine && nbseq != 0u);
        const int tree_lane = treem ? __builtin_ctzll(treem) : -1;
        const int tab_lane = seqm ? __builtin_ctzll(seqm) : -1;
        if (treem & (treem - 1ull))
            bad = true; // a second tree
        if (lessm && (tree_lane < 0 || (lessm & ((1ull << tree_lane) - 1ull))))
            bad = true; // treeless before the tree
        const uint32_t modes0 = tab_lane >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)modes, tab_lane) : 0u;
        {
            uint32_t want = 0;
            for (int t = 0; t < 3; ++t)
            {
                const uint32_t m = (modes0 >> (6 - 2 * t)) & 3u;
                if (m == 3u)
                    bad = true; // nothing to repeat at the head of a piece
                want |= (m ? 3u : 0u) << (6 - 2 * t);
            }
            if (mine && nbseq != 0u && lane != tab_lane && modes != want)
                bad = true;
        }
        if (__builtin_amdgcn_ballot_w64(bad))
            bad = true;
        // ---- the table descriptions (lane 0), the tables (all lanes; their scratch lies over the Huffman table, so:), THEN the tree
        // (lane 0), all by the decoder core's own readers ----
        uint32_t tree_bytes = 0, desc_bytes = 0;
        if (!bad)
        {
            const uint32_t t_off = tree_lane >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)(off + 3u + lhdr), tree_lane) : 0u;
            const uint32_t t_size = tree_lane >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)lcs, tree_lane) : 0u;
            const uint32_t d_off = tab_lane >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)(off + 3u + lhdr + lcs + shdr), tab_lane) : 0u;
            const uint32_t d_end = tab_lane >= 0 ? (uint32_t)__builtin_amdgcn_readlane((int)(off + 3u + csz), tab_lane) : 0u;
            const uint32_t d_staged = d_end - d_off < 512u ? d_end - d_off : 512u, t_staged = t_size < 256u ? t_size : 256u;
            for (uint32_t k = lane; k < d_staged; k += 64)
                s_desc[k] = p[d_off + k];
            for (uint32_t k = lane; k < t_staged; k += 64)
                s_desc[512u + k] = p[t_off + k];
            __syncthreads();
            if (lane == 0)
            {
                sh.v[ZDV_LEN] = 0;
                sh.v[ZDV_LL] = 0;
                if (tab_lane >= 0)
                {
                    uint32_t q = 0; // (a description that ran past the staged bytes fails the readers' bounds checks: the serial decoder then)
                    for (int t = 0; t < 3 && !sh.v[ZDV_ERR]; ++t) // LL, OF, ML
                    {
                        uint32_t used = 0;
                        if (zd_set_table(&sh, t, (modes0 >> (6 - 2 * t)) & 3u, s_desc + q, d_staged - q, &used))
                            sh.v[ZDV_ERR] = 1;
                        q += used;
                    }
                    sh.v[ZDV_LL] = q;
                    if (d_off + q >= d_end)
                        sh.v[ZDV_ERR] = 1;
                }
            }
            __syncthreads();
            bad = sh.v[ZDV_ERR] != 0u;
            desc_bytes = sh.v[ZDV_LL];
            if (!bad && tab_lane >= 0)
            {
                for (int t = 0; t < 3; ++t)
                    if (sh.tb_build[t])
                    {
                        if (zd_build_fse_par(&sh.fse[t], sh.norm + 64 * t, sh.tb_maxsym[t], sh.tb_log[t], sh.cum, (uint32_t*)sh.huf,
                                             sh.huf + 2u * ZD_FSE_PAR_MASK_WORDS, (uint32_t)lane))
                            bad = true;
                        ZB_SYNC_LDS();
                    }
            }
            __syncthreads();
            if (lane == 0 && !bad && tree_lane >= 0)
            {
                const uint32_t tr = zd_read_huf_tree(&sh, s_desc + 512, t_staged);
                if (tr == ZD_ERROR)
                    sh.v[ZDV_ERR] = 1;
                else
                    sh.v[ZDV_LEN] = tr;
            }
            __syncthreads();
            bad = bad || sh.v[ZDV_ERR] != 0u;
            tree_bytes = sh.v[ZDV_LEN];
        }
#ifdef LTHIP_ZB_PROF
        ZB_MARK(20);
#endif
        // ---- literals: offsets, the stream list, raw runs ----
        uint32_t nlit_total, nstr_total, nseq_total;
        const uint32_t lo = z_wave_scan_excl(mine ? nlit : 0u, lane, &nlit_total);
        const bool huf = mine && !raw && lmode >= 2u;
        const uint32_t st0 = z_wave_scan_excl(huf ? nstr : 0u, lane, &nstr_total);
        const uint32_t rec0 = z_wave_scan_excl(mine ? nbseq : 0u, lane, &nseq_total);
        bad = bad || nlit_total > ZD_LIT_MAX || nlit_total > expect;
        if (!bad && huf)
        {
            const uint32_t tb = lane == tree_lane ? tree_bytes : 0u;
            const uint32_t at = off + 3u + lhdr + tb;
            if (lcs < tb)
                bad = true;
            else if (nstr == 1u)
                s_streams[st0] = make_uint4(at, lcs - tb, lo, nlit);
            else if (lcs - tb < 10u)
                bad = true;
            else
            {
                const uint8_t* j = p + at;
                const uint32_t s1 = (uint32_t)j[0] | ((uint32_t)j[1] << 8), s2 = (uint32_t)j[2] | ((uint32_t)j[3] << 8),
                               s3 = (uint32_t)j[4] | ((uint32_t)j[5] << 8);
                const uint32_t body = lcs - tb - 6u, seg = (nlit + 3u) >> 2;
                if (s1 + s2 + s3 >= body || 3u * seg > nlit)
                    bad = true;
                else
                {
                    s_streams[st0] = make_uint4(at + 6u, s1, lo, seg);
                    s_streams[st0 + 1u] = make_uint4(at + 6u + s1, s2, lo + seg, seg);
                    s_streams[st0 + 2u] = make_uint4(at + 6u + s1 + s2, s3, lo + 2u * seg, seg);
                    s_streams[st0 + 3u] = make_uint4(at + 6u + s1 + s2 + s3, body - s1 - s2 - s3, lo + 3u * seg, nlit - 3u * seg);
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(bad))
            bad = true;
        __syncthreads();
        if (!bad)
        {
            // raw / RLE literals and raw blocks: all lanes, unit after unit
            uint64_t plain = __builtin_amdgcn_ballot_w64(mine && nlit != 0u && (raw || lmode < 2u));
            while (plain)
            {
                const int u = __builtin_ctzll(plain);
                plain &= plain - 1ull;
                const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)nlit, u);
                const uint32_t from = (uint32_t)__builtin_amdgcn_readlane((int)(off + 3u + lhdr), u);
                const uint32_t to = (uint32_t)__builtin_amdgcn_readlane((int)lo, u);
                const uint32_t rle = (uint32_t)__builtin_amdgcn_readlane((int)((!raw && lmode == 1u) ? 1u : 0u), u);
                if (rle)
                    for (uint32_t k = lane; k < n; k += 64)
                        lits[to + k] = p[from];
                else
                {
                    typedef uint32_t u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));
                    const uint32_t nv = n >> 4; // 16 bytes per lane and trip, any alignment on both sides
                    for (uint32_t k = lane; k < nv; k += 64)
                        *reinterpret_cast<u32x4_a1*>(lits + to + 16u * k) = *reinterpret_cast<const u32x4_a1*>(p + from + 16u * k);
                    for (uint32_t k = 16u * nv + (uint32_t)lane; k < n; k += 64)
                        lits[to + k] = p[from + k];
                }
            }
            // Huffman streams: TWO per lane, interleaved (a stream is a chain of dependent table reads: two chains hide half of
            // the latency), each with its next 128 bits in registers (ZsWin: no load on the chain).  Four symbols per step while a
            // stream has 64 bits and four symbols left; the core's careful loop finishes it and gives the verdict.
            const uint32_t tl = sh.huf_log;
            for (uint32_t k0 = 0; k0 < nstr_total; k0 += 128u)
            {
                const uint32_t ka = k0 + (uint32_t)lane, kb = ka + 64u;
                const bool has_a = ka < nstr_total, has_b = kb < nstr_total;
                const uint4 sa = has_a ? s_streams[ka] : make_uint4(0, 0, 0, 0), sb2 = has_b ? s_streams[kb] : make_uint4(0, 0, 0, 0);
                uint32_t pa = 0, pb = 0, ia = 0, ib = 0;
                ZsWin wa, wb;
                bool go_a = false, go_b = false;
                if (has_a)
                {
                    const uint32_t last = sa.y ? p[sa.x + sa.y - 1u] : 0u;
                    if (sa.w == 0u || last == 0u)
                        bad = true;
                    else
                    {
                        pa = (sa.y - 1u) * 8u + (31u - (uint32_t)__builtin_clz(last));
                        wa.open(p + sa.x, sa.y, (uint32_t)(it.src_off + sa.x > 64u ? 64u : it.src_off + sa.x));
                        go_a = true;
                    }
                }
                if (has_b)
                {
                    const uint32_t last = sb2.y ? p[sb2.x + sb2.y - 1u] : 0u;
                    if (sb2.w == 0u || last == 0u)
                        bad = true;
                    else
                    {
                        pb = (sb2.y - 1u) * 8u + (31u - (uint32_t)__builtin_clz(last));
                        wb.open(p + sb2.x, sb2.y, (uint32_t)(it.src_off + sb2.x > 64u ? 64u : it.src_off + sb2.x));
                        go_b = true;
                    }
                }
                uint8_t* const oa = lits + sa.z;
                uint8_t* const ob2 = lits + sb2.z;
                for (;;)
                {
                    const bool fa = go_a && sa.w - ia >= 4u && pa >= 64u, fb = go_b && sb2.w - ib >= 4u && pb >= 64u;
                    if (!__builtin_amdgcn_ballot_w64(fa || fb))
                        break;
                    uint64_t ta = 0, tb2 = 0;
                    if (fa)
                    {
                        wa.ensure(pa, 64u);
                        ta = wa.get64(pa - 64u);
                    }
                    if (fb)
                    {
                        wb.ensure(pb, 64u);
                        tb2 = wb.get64(pb - 64u);
                    }
                    uint32_t ua = 0, ub = 0, qa = 0, qb = 0;
#pragma unroll
                    for (uint32_t j = 0; j < 4u; ++j)
                    {
                        const uint32_t ea = sh.huf[(uint32_t)(ta >> (64u - tl))], eb = sh.huf[(uint32_t)(tb2 >> (64u - tl))];
                        const uint32_t na = ea >> 8, nb2 = eb >> 8;
                        ta <<= na;
                        tb2 <<= nb2;
                        ua += na;
                        ub += nb2;
                        qa |= (ea & 255u) << (8u * j);
                        qb |= (eb & 255u) << (8u * j);
                    }
                    if (fa)
                    {
                        __builtin_memcpy(oa + ia, &qa, 4);
                        pa -= ua;
                        ia += 4u;
                    }
                    if (fb)
                    {
                        __builtin_memcpy(ob2 + ib, &qb, 4);
                        pb -= ub;
                        ib += 4u;
                    }
                }
                if (go_a && zd_huf_stream_from(&sh, p + sa.x, sa.y, oa, sa.w, pa, ia))
                    bad = true;
                if (go_b && zd_huf_stream_from(&sh, p + sb2.x, sb2.y, ob2, sb2.w, pb, ib))
                    bad = true;
            }
        }
        if (__builtin_amdgcn_ballot_w64(bad))
            bad = true;
        __syncthreads();
#ifdef LTHIP_ZB_PROF
        ZB_MARK(21);
#endif
        // ---- the tables, packed: one 8-byte read per state ----
        uint32_t log_l = 0, log_o = 0, log_m = 0;
        if (!bad && tab_lane >= 0)
        {
            for (int t = 0; t < 3; ++t)
            {
                const ZdFse* f = &sh.fse[t];
                uint64_t* pk = t == ZT_LL ? pk_ll : t == ZT_ML ? pk_ml : pk_of;
                const uint32_t size = f->valid == 2u ? 1u : f->valid == 1u ? 1u << f->log : 0u;
                if (size == 0u || size > (t == ZT_OF ? 256u : 512u))
                    bad = true;
                const uint32_t lg = f->valid == 2u ? 0u : f->log;
                if (t == ZT_LL)
                    log_l = lg;
                else if (t == ZT_OF)
                    log_o = lg;
                else
                    log_m = lg;
                for (uint32_t x = lane; x < size && !bad; x += 64)
                {
                    const uint32_t sym = f->sym[x];
                    uint32_t baseline, ebits;
                    if (t == ZT_LL)
                    {
                        baseline = zb_ll_base(sym & 63u);
                        ebits = zb_ll_bits(sym & 63u);
                        bad = sym > 35u;
                    }
                    else if (t == ZT_ML)
                    {
                        baseline = zb_ml_base(sym & 63u) + 3u;
                        ebits = zb_ml_bits(sym & 63u);
                        bad = sym > 52u;
                    }
                    else
                    {
                        baseline = 1u << (sym & 31u);
                        ebits = sym & 31u;
                        bad = sym > 31u; // (codes above 23 may sit in a table -- the predefined one has 29 --: a sequence that USES one is stopped in zs_seq_lanes)
                    }
                    // the table's own fields are read before its packed form lands on them?  No: the packed tables lie over the
                    // Huffman table and the weights' table, never over sh.fse
                    pk[x] = (uint64_t)(f->valid == 2u ? 0u : f->base[x]) | ((uint64_t)(f->valid == 2u ? 0u : f->nb[x]) << 16) | ((uint64_t)ebits << 24) |
                            ((uint64_t)baseline << 32);
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(bad))
            bad = true;
        __syncthreads();
#ifdef LTHIP_ZB_PROF
        ZB_MARK(22);
#endif
        // ---- sequences: lane u the bit-stream of block u ----
        uint32_t sum_ll = 0, sum_ml = 0;
        {
            const uint32_t at = off + 3u + lhdr + lcs + shdr + (lane == tab_lane ? desc_bytes : 0u);
            const uint32_t end = off + 3u + csz;
            const bool had = !bad && mine && nbseq != 0u;
            if (it.pad) // (wave-uniform: the frame's trailer version)
                zs_seq_lanes<2>(had, p + at, at < end ? end - at : 0u, (uint32_t)(it.src_off + at > 64u ? 64u : it.src_off + at), nbseq, log_l, log_o,
                                log_m, pk_ll, pk_of, pk_ml, recs + rec0, bad, sum_ll, sum_ml);
            else
                zs_seq_lanes<1>(had, p + at, at < end ? end - at : 0u, (uint32_t)(it.src_off + at > 64u ? 64u : it.src_off + at), nbseq, log_l, log_o,
                                log_m, pk_ll, pk_of, pk_ml, recs + rec0, bad, sum_ll, sum_ml);
            // the block must regenerate exactly its unit
            if (had && !bad && (sum_ll > nlit || nlit + sum_ml != ubytes))
                bad = true;
        }
        if (!bad && mine && nbseq == 0u && nlit != ubytes)
            bad = true; // no sequences: all literals
        if (__builtin_amdgcn_ballot_w64(bad))
            bad = true;
#ifdef LTHIP_ZB_PROF
        ZB_MARK(23);
#endif
        // ---- a block's last literals go with the next sequence of the piece ----
        if (!bad)
        {
            const uint32_t tail = mine ? nlit - sum_ll : 0u;
            uint32_t run = 0, carry = 0;
            for (uint32_t u = 0; u < nunits; ++u)
            {
                const uint32_t tu = (uint32_t)__builtin_amdgcn_readlane((int)tail, (int)u);
                const bool has = (seqm >> u) & 1ull;
                if ((uint32_t)lane == u)
                    carry = run;
                run = has ? tu : run + tu;
            }
            if (mine && nbseq != 0u && carry != 0u)
                recs[rec0] += carry; // (20 bits hold a whole piece of literals)
        }
        ZPrep pr;
        pr.bits_off = 0;
        pr.bits_size = 0;
        pr.nbseq = nseq_total;
        pr.nlit = nlit_total;
        pr.log[0] = pr.log[1] = pr.log[2] = 0;
        pr.expect = expect;
        pr.status = bad ? ZP_SERIAL : ZP_READY;
        if (lane == 0)
        {
            prep[i] = pr;
            if (bad)
                retry[it.payload] = 1u;
        }
    }
}

