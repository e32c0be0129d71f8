// zd_foreign_blocks.inc -- part of k_zstd_decode.hip (one translation unit; included there, inside its anonymous namespace, in this order):
// frames of other encoders, block-parallel entropy stage -- k_zstd_blk_entropy / k_zstd_blk_sequences, plain pieces, the serial retry
// ---------------------------------------------------------------------------------------------------
// Frames of other encoders, block-parallel (fitems, kind 4): k_zstd_blk_entropy, one wave per BLOCK.
// A block's streams need nothing from the blocks before it except their entropy tables (Treeless literals, Repeat_Mode), and those
// are found without decoding anything: the wave walks the headers of the blocks before its own (section headers only), notes which
// block last SET the Huffman tree and each of the three FSE tables, and builds them from there with the decoder core's readers.
// Then it decodes its own block's literal streams (two per lane) into the block's literal buffer and its sequence bit-stream (one
// lane) into records -- offset values 1..3 (repeat offsets) stay in the records; k_zstd_execute<2> resolves them when it executes
// the payload's blocks in order.  Whatever is unusual gives the payload back to the serial decoder.
// ---------------------------------------------------------------------------------------------------
struct ZfBlk
{
    uint32_t lmode, nlit, lhdr, lcs, nstr, nbseq, shdr, modes;
    bool ok;
};
// section headers of a Compressed_Block's content c[0 .. csz)
__device__ __forceinline__ ZfBlk zf_parse(const uint8_t* c, uint32_t csz)
{
    ZfBlk f;
    f.lmode = f.nlit = f.lhdr = f.lcs = f.nstr = f.nbseq = f.shdr = f.modes = 0;
    f.ok = false;
    if (csz < 2u)
        return f;
    const uint32_t b0 = c[0], sf = (b0 >> 2) & 3u;
    f.lmode = b0 & 3u;
    if (f.lmode < 2u)
    {
        f.lhdr = (sf & 1u) == 0u ? 1u : sf == 1u ? 2u : 3u;
        if (f.lhdr > csz)
            return f;
        f.nlit = f.lhdr == 1u ? b0 >> 3 : f.lhdr == 2u ? ((uint32_t)c[0] | ((uint32_t)c[1] << 8)) >> 4
                                                       : ((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16)) >> 4;
        f.lcs = f.lmode == 0u ? f.nlit : 1u;
    }
    else
    {
        f.lhdr = sf < 2u ? 3u : sf == 2u ? 4u : 5u;
        if (f.lhdr > csz)
            return f;
        if (f.lhdr == 3u)
        {
            const uint32_t hh = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
            f.nlit = (hh >> 4) & 0x3FFu;
            f.lcs = hh >> 14;
        }
        else if (f.lhdr == 4u)
        {
            const uint32_t hh = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
            f.nlit = (hh >> 4) & 0x3FFFu;
            f.lcs = hh >> 18;
        }
        else
        {
            const uint32_t hh = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
            f.nlit = (hh >> 4) & 0x3FFFFu;
            f.lcs = (hh >> 22) | ((uint32_t)c[4] << 10);
        }
        f.nstr = sf == 0u ? 1u : 4u;
    }
    if (f.nlit > ZD_LIT_MAX || f.lcs >= csz - f.lhdr) // (at least one byte of sequences section follows)
        return f;
    const uint32_t sp = f.lhdr + f.lcs;
    const uint32_t n0 = c[sp];
    if (n0 == 0u)
    {
        f.shdr = 1;
        f.ok = sp + 1u == csz;
        return f;
    }
    if (n0 < 128u)
    {
        f.nbseq = n0;
        f.shdr = 1;
    }
    else if (n0 < 255u)
    {
        if (sp + 2u > csz)
            return f;
        f.nbseq = ((n0 - 128u) << 8) + c[sp + 1u];
        f.shdr = 2;
    }
    else
    {
        if (sp + 3u > csz)
            return f;
        f.nbseq = (uint32_t)c[sp + 1u] + ((uint32_t)c[sp + 2u] << 8) + 0x7F00u;
        f.shdr = 3;
    }
    if (sp + f.shdr + 1u >= csz || f.nbseq == 0u)
        return f;
    f.modes = c[sp + f.shdr];
    f.shdr += 1u;
    f.ok = (f.modes & 3u) == 0u;
    return f;
}

// Room in an arena (a counter that only grows, up to `cap`): a draw that does not fit leaves the counter as it was, so a block too
// dense for the arena sends its own payload to the serial decoder and the other payloads of the call keep their room.
__device__ __forceinline__ bool zf_draw(unsigned long long* counter, unsigned long long want, unsigned long long cap, unsigned long long* at)
{
    unsigned long long old = atomicAdd(counter, 0ull); // (the counter itself, not a cached copy: a draw may have been given back)
    for (;;)
    {
        if (old + want > cap)
            return false;
        const unsigned long long seen = atomicCAS(counter, old, old + want);
        if (seen == old)
        {
            *at = old;
            return true;
        }
        old = seen;
    }
}

__global__ __launch_bounds__(64) void k_zstd_blk_entropy(const uint8_t* __restrict__ src, const ZItem* __restrict__ fitems, const uint32_t* __restrict__ flist,
                                                         uint32_t nlist, uint32_t* __restrict__ slist, uint32_t* __restrict__ scount,
                                                         uint8_t* __restrict__ lit_scratch, uint64_t* __restrict__ rec_scratch,
                                                         ZPrep* __restrict__ fprep, uint32_t* __restrict__ retry, uint32_t* __restrict__ ticket,
                                                         unsigned long long* __restrict__ bump, uint64_t lit_cap, uint64_t rec_cap,
                                                         uint64_t* __restrict__ tabs, uint32_t inline_seqs)
{
    __shared__ ZdShared sh;
    __shared__ uint4 s_streams[4];
    __shared__ __attribute__((aligned(16))) uint8_t s_desc[512 + 256];
    const int lane = threadIdx.x;
    uint64_t* const pk_ll = reinterpret_cast<uint64_t*>(sh.huf);
    uint64_t* const pk_ml = pk_ll + 512;
    uint64_t* const pk_of = reinterpret_cast<uint64_t*>(&sh.wtab);
    for (;;)
    {
        __builtin_amdgcn_wave_barrier();
        uint32_t tk = atomicAdd(ticket, lane == 0 ? 1u : 0u);
        tk = __builtin_amdgcn_readfirstlane(tk);
        if (tk >= nlist)
            break;
        const uint32_t i = flist[tk];
        const ZItem it = fitems[i];
        if (it.kind != 4u)
            continue;
        __syncthreads();
#ifdef LTHIP_ZB_PROF
        if (lane == 0)
            g_zb_last[blockIdx.x] = wall_clock64();
#endif
        const uint8_t* p = src + it.src_off; // the payload
        ZPrep pr;
        pr.bits_off = 0;
        pr.bits_size = pr.nbseq = pr.nlit = 0;
        pr.log[0] = pr.log[1] = pr.log[2] = 0;
        pr.expect = 0;
        pr.status = ZP_SERIAL;
        pr.rec_at = 0;
        pr.seq_off = pr.seq_size = 0;
        uint32_t why = 0;
        bool bad = false;
        if (lane == 0)
        {
            sh.v[ZDV_ERR] = 0;
            sh.v[ZDV_PREP] = 0;
            sh.huf_valid = 0;
        }
        const uint32_t bh = (uint32_t)p[it.pad] | ((uint32_t)p[it.pad + 1u] << 8) | ((uint32_t)p[it.pad + 2u] << 16);
        const uint32_t type = (bh >> 1) & 3u, bsize = bh >> 3;
        if (type != 2u)
        {
            // Raw_Block / RLE_Block: where the bytes are (the executor copies / fills)
            pr.log[0] = type == 0u ? 1u : 2u;
            pr.bits_off = it.src_off + it.pad + 3u;
            pr.expect = bsize;
            pr.status = ZP_DONE;
            if (lane == 0)
                fprep[i] = pr;
            continue;
        }
        const uint32_t c0 = it.pad + 3u; // my block's content inside the payload
        const ZfBlk me = zf_parse(p + c0, bsize);
        bad = !me.ok;
        // room for my literals and my records in the two arenas (a wave-uniform draw; an arena that is full sends the payload to the
        // serial decoder: the host sizes them for a record per six bytes of output)
        unsigned long long lit_at = 0, rec_at = 0;
        if (!bad)
        {
            const unsigned long long want_l = ((unsigned long long)me.nlit + 79ull) & ~15ull;
            uint32_t fits = 0;
            if (lane == 0)
            {
                // the literals first (a damaged header can state at most 2^18 of them), then the records; a block whose records do
                // not fit gives its literals' room back if nobody has drawn behind it
                if (zf_draw(&bump[0], want_l, lit_cap, &lit_at))
                {
                    if (zf_draw(&bump[1], me.nbseq, rec_cap, &rec_at))
                        fits = 1;
                    else
                        (void)atomicCAS(&bump[0], lit_at + want_l, lit_at);
                }
            }
            fits = __builtin_amdgcn_readfirstlane(fits);
            lit_at = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(lit_at >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)lit_at);
            rec_at = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(rec_at >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)rec_at);
            if (!fits)
                { bad = true; why = __LINE__; }
        }
        uint8_t* lits = lit_scratch + lit_at;
        // ---- who set the tree / the tables last?  (the section headers of the blocks up to mine) ----
        uint32_t tree_at = 0, tree_size = 0, tab_at[3] = {0, 0, 0}, tab_end[3] = {0, 0, 0}, tab_modes[3] = {0, 0, 0};
        bool have_tree = false, have_tab[3] = {false, false, false};
        if (!bad)
        {
            const ZFrameHdr fh = z_frame_header(p, it.size);
            uint32_t q = fh.size;
            for (uint32_t j = 0; j <= it.aux && !bad; ++j)
            {
                const uint32_t h = (uint32_t)p[q] | ((uint32_t)p[q + 1u] << 8) | ((uint32_t)p[q + 2u] << 16);
                const uint32_t ty = (h >> 1) & 3u, sz = h >> 3;
                if (ty == 2u)
                {
                    const ZfBlk f = j == it.aux ? me : zf_parse(p + q + 3u, sz);
                    if (!f.ok)
                        { bad = true; why = __LINE__; }
                    else
                    {
                        if (f.lmode == 2u)
                        {
                            have_tree = true;
                            tree_at = q + 3u + f.lhdr;
                            tree_size = f.lcs;
                        }
                        if (f.nbseq)
                            for (int t = 0; t < 3; ++t)
                                if (((f.modes >> (6 - 2 * t)) & 3u) != 3u)
                                {
                                    have_tab[t] = true;
                                    tab_at[t] = q + 3u + f.lhdr + f.lcs + f.shdr; // the first description of that block
                                    tab_end[t] = q + 3u + sz;
                                    tab_modes[t] = f.modes;
                                }
                    }
                }
                q += 3u + (ty == 1u ? 1u : sz);
            }
            if ((me.lmode == 3u && !have_tree) || (me.nbseq && !(have_tab[0] && have_tab[1] && have_tab[2])))
                { bad = true; why = __LINE__; } // nothing to repeat: the serial decoder says so
        }
#ifdef LTHIP_ZB_PROF
        ZB_MARK(19);
#endif
        // ---- the three tables (descriptions by lane 0 from staged bytes, tables by all lanes), then the tree ----
        if (!bad && me.nbseq)
        {
            for (int t = 0; t < 3 && !bad; ++t)
            {
                const uint32_t staged = tab_end[t] - tab_at[t] < 512u ? tab_end[t] - tab_at[t] : 512u;
                __syncthreads();
                for (uint32_t k = lane; k < staged; k += 64)
                    s_desc[k] = p[tab_at[t] + k];
                __syncthreads();
                if (lane == 0)
                {
                    // the descriptions of a block lie one behind the other (LL, OF, ML): skip the ones before mine
                    uint32_t q = 0;
                    for (int tt = 0; tt <= t && !sh.v[ZDV_ERR]; ++tt)
                    {
                        const uint32_t m = (tab_modes[t] >> (6 - 2 * tt)) & 3u;
                        uint32_t used = 0;
                        if ((m == 1u || m == 2u) && q >= staged) // a description past what was staged (also the one-byte RLE form):
                        {                                        // `staged - q` must never wrap -- the payload goes to the serial decoder
                            sh.v[ZDV_ERR] = 1;
                            break;
                        }
                        if (tt == t)
                        {
                            if (zd_set_table(&sh, t, m, s_desc + q, staged - q, &used))
                                sh.v[ZDV_ERR] = 1;
                        }
                        else if (m == 1u)
                            used = 1;
                        else if (m == 2u)
                        {
                            uint32_t maxsym = tt == ZT_LL ? 35u : tt == ZT_ML ? 52u : 31u, tl = 0;
                            used = q < staged ? zd_read_ncount(s_desc + q, staged - q, sh.norm + 192, &maxsym, zb_table_max_log(tt), &tl) : ZD_ERROR;
                            if (used == ZD_ERROR)
                            {
                                sh.v[ZDV_ERR] = 1;
                                used = 0;
                            }
                        }
                        q += used;
                        if (q > staged)
                            sh.v[ZDV_ERR] = 1;
                    }
                }
                __syncthreads();
                bad = sh.v[ZDV_ERR] != 0u;
                if (!bad && sh.tb_build[t])
                {
                    if (zd_build_fse_par(&sh.fse[t], sh.norm + 64 * t, sh.tb_maxsym[t], sh.tb_log[t], sh.cum, (uint32_t*)sh.huf,
                                         sh.huf + 2u * ZD_FSE_PAR_MASK_WORDS, (uint32_t)lane))
                        { bad = true; why = __LINE__; }
                    ZB_SYNC_LDS();
                }
            }
            __syncthreads();
        }
        uint32_t tree_bytes = 0;
        if (!bad && me.lmode >= 2u)
        {
            const uint32_t staged = tree_size < 256u ? tree_size : 256u;
            for (uint32_t k = lane; k < staged; k += 64)
                s_desc[512u + k] = p[tree_at + k];
            __syncthreads();
            if (lane == 0)
            {
                const uint32_t tr = zd_read_huf_tree(&sh, s_desc + 512, staged);
                if (tr == ZD_ERROR)
                    sh.v[ZDV_ERR] = 1;
                else
                    sh.v[ZDV_LEN] = tr;
            }
            __syncthreads();
            bad = sh.v[ZDV_ERR] != 0u;
            tree_bytes = me.lmode == 2u ? sh.v[ZDV_LEN] : 0u;
        }
#ifdef LTHIP_ZB_PROF
        ZB_MARK(20);
#endif
        // ---- literals ----
        uint32_t nstr_total = 0;
        if (!bad)
        {
            const uint32_t at0 = c0 + me.lhdr;
            if (me.lmode == 0u)
            {
                typedef uint32_t u32x4_a1 __attribute__((ext_vector_type(4), aligned(1)));
                const uint32_t nv = me.nlit >> 4;
                for (uint32_t k = lane; k < nv; k += 64)
                    *reinterpret_cast<u32x4_a1*>(lits + 16u * k) = *reinterpret_cast<const u32x4_a1*>(p + at0 + 16u * k);
                for (uint32_t k = 16u * nv + (uint32_t)lane; k < me.nlit; k += 64)
                    lits[k] = p[at0 + k];
            }
            else if (me.lmode == 1u)
                for (uint32_t k = lane; k < me.nlit; k += 64)
                    lits[k] = p[at0];
            else
            {
                const uint32_t at = at0 + tree_bytes;
                if (me.lcs < tree_bytes)
                    { bad = true; why = __LINE__; }
                else if (me.nstr == 1u)
                {
                    if (lane == 0)
                        s_streams[0] = make_uint4(at, me.lcs - tree_bytes, 0u, me.nlit);
                    nstr_total = 1;
                }
                else if (me.lcs - tree_bytes < 10u)
                    { bad = true; why = __LINE__; }
                else
                {
                    const uint8_t* j = p + at;
                    const uint32_t s1 = (uint32_t)j[0] | ((uint32_t)j[1] << 8), s2 = (uint32_t)j[2] | ((uint32_t)j[3] << 8),
                                   s3 = (uint32_t)j[4] | ((uint32_t)j[5] << 8);
                    const uint32_t body = me.lcs - tree_bytes - 6u, seg = (me.nlit + 3u) >> 2;
                    if (s1 + s2 + s3 >= body || 3u * seg > me.nlit)
                        { bad = true; why = __LINE__; }
                    else
                    {
                        if (lane == 0)
                        {
                            s_streams[0] = make_uint4(at + 6u, s1, 0u, seg);
                            s_streams[1] = make_uint4(at + 6u + s1, s2, seg, seg);
                            s_streams[2] = make_uint4(at + 6u + s1 + s2, s3, 2u * seg, seg);
                            s_streams[3] = make_uint4(at + 6u + s1 + s2 + s3, body - s1 - s2 - s3, 3u * seg, me.nlit - 3u * seg);
                        }
                        nstr_total = 4;
                    }
                }
            }
        }
        __syncthreads();
        if (!bad && nstr_total)
        {
            // the streams: one per lane (a block has at most four; the loop is k_zstd_sub_entropy's, its second stream unused: this
            // wave has lanes to spare, and a lane alone with one chain finishes it sooner than two lanes with two chains each)
            const uint32_t tl = sh.huf_log;
            const uint32_t ka = (uint32_t)lane, kb = ka + 64u;
            const bool has_a = ka < nstr_total, has_b = kb < nstr_total;
            const uint4 sa = has_a ? s_streams[ka] : make_uint4(0, 0, 0, 0), sb2 = has_b ? s_streams[kb] : make_uint4(0, 0, 0, 0);
            uint32_t pa = 0, pb = 0, ia = 0, ib = 0;
            ZsWin wa, wb;
            wa.base = wb.base = p;
            wa.hi = wa.lo = wa.nx = wb.hi = wb.lo = wb.nx = 0;
            wa.top = wb.top = 0;
            wa.reach = wb.reach = 0;
            bool go_a = false, go_b = false;
            if (has_a)
            {
                const uint32_t last = sa.y ? p[sa.x + sa.y - 1u] : 0u;
                if (sa.w == 0u || last == 0u)
                    { bad = true; why = __LINE__; }
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
                    { bad = true; why = __LINE__; }
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
                { bad = true; why = __LINE__; }
            if (go_b && zd_huf_stream_from(&sh, p + sb2.x, sb2.y, ob2, sb2.w, pb, ib))
                { bad = true; why = __LINE__; }
        }
        if (__builtin_amdgcn_ballot_w64(bad))
            { bad = true; why = __LINE__; }
        __syncthreads();
#ifdef LTHIP_ZB_PROF
        ZB_MARK(21);
#endif
        // ---- the tables, packed; the sequences (lane 0) ----
        uint32_t log_l = 0, log_o = 0, log_m = 0, seq_ml = 0;
        if (!bad && me.nbseq)
        {
            for (int t = 0; t < 3; ++t)
            {
                const ZdFse* f = &sh.fse[t];
                uint64_t* pk = t == ZT_LL ? pk_ll : t == ZT_ML ? pk_ml : pk_of;
                const uint32_t size = f->valid == 2u ? 1u : f->valid == 1u ? 1u << f->log : 0u;
                if (size == 0u || size > (t == ZT_OF ? 256u : 512u))
                    { bad = true; why = __LINE__; }
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
                    pk[x] = (uint64_t)(f->valid == 2u ? 0u : f->base[x]) | ((uint64_t)(f->valid == 2u ? 0u : f->nb[x]) << 16) | ((uint64_t)ebits << 24) |
                            ((uint64_t)baseline << 32);
                }
            }
            if (__builtin_amdgcn_ballot_w64(bad))
                { bad = true; why = __LINE__; }
            __syncthreads();
            const uint32_t at = c0 + me.lhdr + me.lcs + me.shdr + (uint32_t)0;
            // my own block's descriptions precede the bit-stream: their size = the bytes its non-repeated tables took
            uint32_t skip = 0;
            if (!bad)
            {
                if (lane == 0)
                {
                    uint32_t q = 0;
                    const uint32_t avail = c0 + bsize - at;
                    for (int tt = 0; tt < 3 && !sh.v[ZDV_ERR]; ++tt)
                    {
                        const uint32_t m = (me.modes >> (6 - 2 * tt)) & 3u;
                        if (m == 1u)
                            q += 1u;
                        else if (m == 2u)
                        {
                            uint32_t maxsym = tt == ZT_LL ? 35u : tt == ZT_ML ? 52u : 31u, tl2 = 0;
                            const uint32_t used = q < avail ? zd_read_ncount(p + at + q, avail - q, sh.norm + 192, &maxsym, zb_table_max_log(tt), &tl2) : ZD_ERROR;
                            if (used == ZD_ERROR)
                                sh.v[ZDV_ERR] = 1;
                            else
                                q += used;
                        }
                    }
                    sh.v[ZDV_LL] = q;
                    if (q >= avail)
                        sh.v[ZDV_ERR] = 1;
                }
                __syncthreads();
                bad = sh.v[ZDV_ERR] != 0u;
                skip = sh.v[ZDV_LL];
            }
            const uint32_t sat = at + skip, send = c0 + bsize;
            // the packed tables go to the block's place in the table arena: k_zstd_blk_sequences decodes the bit-streams of 64 blocks
            // per wave, a lane each, reading its states' entries from there.  ONE lane of this wave takes 2.3 ms per block with the
            // tables in shared memory -- which is the faster way as long as the call has no more blocks than the machine has waves for
            // (a lane of k_zstd_blk_sequences takes 14 ms for its block, however few there are): inline_seqs.
            if (!bad && inline_seqs)
            {
                uint32_t sum_ll = 0, sum_ml = 0;
                zs_seq_lanes<0>(lane == 0, p + sat, sat < send ? send - sat : 0u, (uint32_t)(it.src_off + sat > 64u ? 64u : it.src_off + sat),
                                    me.nbseq, log_l, log_o, log_m, pk_ll, pk_of, pk_ml, rec_scratch + rec_at, bad, sum_ll, sum_ml);
                sum_ll = (uint32_t)__builtin_amdgcn_readfirstlane(sum_ll);
                sum_ml = (uint32_t)__builtin_amdgcn_readfirstlane(sum_ml);
                if (__builtin_amdgcn_ballot_w64(bad))
                    bad = true;
                if (!bad && (sum_ll > me.nlit || me.nlit + sum_ml > ZB))
                    bad = true;
                seq_ml = sum_ml;
            }
            else if (!bad)
            {
                // (its place in the table arena = its place in the list of blocks k_zstd_blk_sequences has to visit)
                uint32_t si = atomicAdd(scount, lane == 0 ? 1u : 0u);
                si = __builtin_amdgcn_readfirstlane(si);
                if (lane == 0)
                    slist[si] = i;
                uint64_t* tp = tabs + (uint64_t)si * 1280u;
                for (uint32_t x = lane; x < 512u; x += 64)
                {
                    tp[x] = pk_ll[x];
                    tp[512u + x] = pk_ml[x];
                }
                for (uint32_t x = lane; x < 256u; x += 64)
                    tp[1024u + x] = pk_of[x];
                pr.seq_off = sat;
                pr.seq_size = sat < send ? send - sat : 0u;
                pr.log[1] = log_l | (log_o << 8) | (log_m << 16);
            }
        }
        else if (!bad && me.nlit > ZB)
            { bad = true; why = __LINE__; }
#ifdef LTHIP_ZB_PROF
        ZB_MARK(23);
#endif
        pr.nbseq = me.nbseq;
        pr.nlit = me.nlit;
        pr.expect = me.nlit + seq_ml; // (k_zstd_blk_sequences adds the match lengths when the sequences are its)
        pr.bits_off = lit_at;
        pr.rec_at = rec_at;
        pr.status = bad ? ZP_SERIAL : ZP_READY;
        if (lane == 0)
        {
            fprep[i] = pr;
            if (bad)
                retry[it.payload] = why ? why : __LINE__;
        }
    }
}

// The sequence bit-streams of other encoders' blocks: 64 blocks per wave, a lane each (zs_seq_lanes), every lane reading the entries of
// ITS block's tables from the table arena (three 8-byte gathers per sequence: the machine has the lanes and the L2 for them; one lane
// with its tables in shared memory, the other 63 idle, is what made k_zstd_blk_entropy take 2.3 ms per block).
__global__ __launch_bounds__(64) void k_zstd_blk_sequences(const uint8_t* __restrict__ src, const ZItem* __restrict__ fitems, const uint32_t* __restrict__ slist,
                                                          const uint32_t* __restrict__ scount,
                                                          const uint64_t* __restrict__ tabs, uint64_t* __restrict__ rec_scratch,
                                                          ZPrep* __restrict__ fprep, uint32_t* __restrict__ retry)
{
    const uint32_t g = blockIdx.x * 64u + threadIdx.x;
    if (blockIdx.x * 64u >= *scount)
        return;
    ZItem it;
    it.kind = 0;
    it.src_off = 0;
    it.payload = 0;
    uint32_t i = 0;
    if (g < *scount)
    {
        i = slist[g];
        it = fitems[i];
    }
    ZPrep pr;
    pr.status = ZP_SERIAL;
    pr.nbseq = pr.nlit = pr.seq_off = pr.seq_size = 0;
    pr.log[0] = 1;
    pr.log[1] = 0;
    pr.rec_at = 0;
    if (it.kind == 4u)
        pr = fprep[i];
    const bool act = it.kind == 4u && pr.status == ZP_READY && pr.log[0] == 0u && pr.nbseq != 0u;
    const uint64_t* tp = tabs + (uint64_t)g * 1280u;
    bool bad = false;
    uint32_t sum_ll = 0, sum_ml = 0;
    const uint64_t at = it.src_off + pr.seq_off;
    zs_seq_lanes<0>(act, src + at, pr.seq_size, (uint32_t)(at > 64u ? 64u : at), pr.nbseq, pr.log[1] & 255u, (pr.log[1] >> 8) & 255u,
                        (pr.log[1] >> 16) & 255u, tp, tp + 1024, tp + 512, rec_scratch + pr.rec_at, bad, sum_ll, sum_ml);
    if (act)
    {
        if (!bad && (sum_ll > pr.nlit || pr.nlit + sum_ml > ZB))
            bad = true;
        if (bad)
        {
            fprep[i].status = ZP_SERIAL;
            retry[it.payload] = __LINE__;
        }
        else
            fprep[i].expect = pr.nlit + sum_ml; // what the block regenerates
    }
}

// Pieces of directory frames that are ONE Raw_Block or RLE_Block (kind 2 with aux != 0: k_zstd_split has checked the header against
// the directory): a copy / a fill, 256 threads per piece -- no reason to send them through the decoder core.
__global__ __launch_bounds__(256) void k_zstd_plain_pieces(const uint8_t* __restrict__ src, const ZBlock* __restrict__ blocks, const ZItem* __restrict__ items,
                                                           const uint32_t* __restrict__ item_count, uint32_t item0, uint32_t item1,
                                                           uint8_t* __restrict__ dst, ZPrep* __restrict__ prep, const uint32_t* __restrict__ perm)
{
    if (item0 + blockIdx.x >= item1 || item0 + blockIdx.x >= *item_count)
        return;
    const uint32_t i = perm[item0 + blockIdx.x];
    const ZItem it = items[i];
    if (it.kind != 2u || it.aux == 0u)
        return;
    const ZBlock blk = blocks[it.payload];
    const uint8_t* p = src + it.src_off;
    const uint32_t bh = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    const uint32_t len = bh >> 3;
    uint8_t* out = dst + blk.dst_off + it.out0;
    if ((uint64_t)it.out0 + len > (uint64_t)blk.dst_cap)
        return; // (cannot happen: the content size fits the capacity; the piece then stays for the serial piece decoder)
    if (((bh >> 1) & 3u) == 1u)
    {
        const uint8_t b = p[3];
        for (uint32_t k = threadIdx.x; k < len; k += 256)
            out[k] = b;
    }
    else
        wg_copy16(out, p + 3, len, threadIdx.x);
    if (threadIdx.x == 0)
    {
        ZPrep pr;
        pr.bits_off = 0;
        pr.bits_size = pr.nbseq = pr.nlit = 0;
        pr.log[0] = pr.log[1] = pr.log[2] = 0;
        pr.expect = len;
        pr.status = ZP_DONE;
        prep[i] = pr;
    }
}

// payloads the sub-block decoder gave back: the whole payload, serially (the plain decoder's verdict and bytes)
__global__ __launch_bounds__(64) void k_zstd_decode_retry(const uint8_t* __restrict__ src, const ZBlock* __restrict__ blocks, uint32_t nblocks,
                                                          const uint32_t* __restrict__ retry, uint8_t* __restrict__ dst,
                                                          uint8_t* __restrict__ lit_scratch, uint32_t* __restrict__ out_sizes)
{
    __shared__ ZdShared sh;
    uint8_t* lits = lit_scratch + (uint64_t)blockIdx.x * (ZD_LIT_MAX + 64u);
    if (threadIdx.x == 0)
        sh.v[ZDV_PREP] = 0;
    for (uint32_t b = blockIdx.x; b < nblocks; b += gridDim.x)
    {
        if (!retry[b])
            continue;
        const ZBlock blk = blocks[b];
        __syncthreads();
        const uint32_t n = zd_decode_payload_ex(src + blk.src_off, blk.size, dst + blk.dst_off, blk.dst_cap, lits, &sh, threadIdx.x, ZD_WHOLE);
        if (threadIdx.x == 0)
            out_sizes[b] = n;
        __syncthreads();
    }
}

