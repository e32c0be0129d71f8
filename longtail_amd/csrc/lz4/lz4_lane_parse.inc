// lz4_lane_parse.inc -- part of k_lz4.hip (one translation unit; included there, inside its anonymous namespace, in this order):
// the lane-sequential parse of one 4 KiB unit by one wave (lz4_lane_parse2): probe, extension, records, cover scans, emission
// ---------------------------------------------------------------------------------------------------
// K5, lane-sequential parse (MODE 1).  The batch parser above looks at 64 CONSECUTIVE positions per step and then has to choose
// among the hits -- a scalar walk that costs ~400 wave instructions per 64 positions on compressible data.  Here every lane owns
// a SUB-UNIT (unit / 64 bytes) and runs the reference's greedy loop on it (lz4.c:1019-1110: probe; on a hit extend, record,
// jump; else step one byte): 64 independent parsers in lock step, one probe per lane per iteration, no selection at all.
//   * the table is the wave's private one; positions of all lanes go into it.  Lanes are mapped to sub-units in REVERSE
//     (lane 63 = first sub-unit) so that when two lanes write one slot in the same instruction the surviving entry is the lower
//     position, which every later sub-unit can use (tools/lz4_lane_model.c: "lines" 8.4 -> 20.7, mixed 1.66 -> 1.72)
//   * a match may run past its lane's sub-unit (up to the unit's end); what it covers is dropped from the later lanes'
//     records afterwards (exclusive prefix maximum of the lanes' match ends) and lanes that are covered while a long match
//     is being extended stop parsing
//   * records {start, length, offset} stay in registers (8 per lane); after the parse three wave scans (cover, previous kept
//     end, output offset) place every lane's sequences and each lane writes its own bytes; literal runs longer than 16 bytes
//     are copied by the whole wave
// Results are a function of the data only (the table is private, the wave runs in lock step).
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t LZ4_LANE_MAXREC = 8; // sequences a lane may record (tools/lz4_lane_model.c: 8 costs nothing, 6 does)

#ifdef LTHIP_K5_PROF /* debug build only (make prof, tools/k5_prof.sh): shader-clock cycles per phase of the lane parser, summed over all waves */
__device__ unsigned long long g_k5_prof[32];
struct K5Prof
{
    unsigned long long last, acc[16];
};
#define K5P_DECL K5Prof k5p; k5p.last = __builtin_readcyclecounter(); for (int i__ = 0; i__ < 16; ++i__) k5p.acc[i__] = 0;
#define K5P_ARG , K5Prof& k5p
#define K5P_PASS , k5p
#define K5P(i) do { const unsigned long long n__ = __builtin_readcyclecounter(); k5p.acc[i] += n__ - k5p.last; k5p.last = n__; } while (0)
#define K5P_COUNT(i, n) do { k5p.acc[i] += (n); } while (0)
#define K5P_FLUSH do { if ((threadIdx.x & 63) == 0) for (int i__ = 0; i__ < 16; ++i__) atomicAdd(&g_k5_prof[i__], k5p.acc[i__]); } while (0)
#else
#define K5P_DECL
#define K5P_ARG
#define K5P_PASS
#define K5P(i) do { } while (0)
#define K5P_COUNT(i, n) do { } while (0)
#define K5P_FLUSH do { } while (0)
#endif

// Scans in SUB-UNIT order with the reverse mapping (sub-unit 63 - lane): a prefix over the sub-units is a SUFFIX over the lanes.  Round 5:
// with DPP moves -- four row shifts inside the rows of 16 (a lane takes the value n lanes above it; beyond the row: nothing), then the
// rows above a lane's row through three v_readlane -- instead of six ds_bpermute round trips with their index arithmetic (36 vector
// instructions and six LDS operations a scan; the three or four scans behind a unit's parse were 3 % of the kernel).
template <bool MAX>
__device__ __forceinline__ uint32_t lane_suffix_scan(uint32_t v, int lane)
{
    auto op = [](uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : a + b; };
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, true)); // row_shl:1
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x102, 0xf, 0xf, true)); // row_shl:2
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xf, 0xf, true)); // row_shl:4
    v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x108, 0xf, 0xf, true)); // row_shl:8
    // a row's first lane holds the row: rows above mine
    const uint32_t t1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16), t2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32),
                   t3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    const uint32_t s1 = op(t2, t3), s0 = op(t1, s1);
    const uint32_t above = lane < 16 ? s0 : (lane < 32 ? s1 : (lane < 48 ? t3 : 0u));
    return op(v, above);
}
// the value of the sub-unit before mine (the lane above; the first sub-unit: 0)
__device__ __forceinline__ uint32_t lane_from_sub_before(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true); // wave_shl:1
}

// ---------------------------------------------------------------------------------------------------
// K5, lane-sequential parse, second formulation (round 4).  The parse is the one described above -- the probe rule, candidates,
// extension limits and cover rule of round 3's formulation: the payloads are byte-identical -- restated around what the per-phase
// cycle counters said it costs (profiles/r04_k5_prof.txt: a probe step took 1500 cycles for ~100 instructions):
//   * PROBE in three LDS round trips instead of four: the private and the shared candidate's bytes are read by ONE pair of
//     unconditional reads (an invalid candidate reads the lane's own position and is masked) -- the compiler had serialised the two
//     predicated reads, each with its own s_waitcnt.  (Round 4 also kept the lane's next bytes in a three-dword register window that
//     slid with p, for two round trips; round 5 took it out again: the kernel had become bound by the number of instructions it
//     issues, and the window's bookkeeping was a fifth of the probe round's.)
//   * EXTENSION in one round trip: the 28 bytes p-8 .. p+20 of both sides are eight aligned dwords each (the window is staged 16
//     bytes into LDS so that "8 bytes before position 0" is a legal address), read together; the backward count and the first 16
//     forward bytes come out of the same registers.  Matches of 20 bytes and more take a second 16-byte round, then the wave.
//   * RECORDS in registers (8 x {start | length << 16, offset}) instead of a global scratch area of 4 KiB per unit that the cover
//     scans, the size pass and the emission each read back through the memory system (1 B/B written and read on "tokens").
// Round 5 (DESIGN.md §6, row r05n; tools/isa_blocks.py): the same parse, byte for byte, in a quarter fewer instructions -- vector AND
// scalar, which issue at the same aggregate rate.  The rules that came out of it: a ballot wants ONE compare (a combination of
// conditions costs a select and a second compare); wave-uniform state wants the scalar unit; switches of experiments want to be
// compile-time zeros in the product; code that every wave walks anyway wants | and & and selects instead of || / && / else-if (an
// exec-mask region is three scalar instructions), code that whole waves usually skip wants the branch.
// ---------------------------------------------------------------------------------------------------
constexpr uint32_t LZ4_LPAD = 16; // LDS byte offset of the staged window
constexpr uint32_t LZ4_QUIET = 3;  // lane parser: probe rounds without a hit at an unaligned position before the one-byte steps stop
                                   // (profiles/r05_adaptive_stepping.txt: 6 / 4 / 3 / 2 / 1 rounds: match finder 161.6 / 160.3 / 159.0 / 158.1 /
                                   // 156.4 ms per 64 GiB of "mixed", word-soup text 2.0284 / 2.0284 / 2.0283 / 2.0282 / 2.0249; fixed rule 169.9, 2.0284)
constexpr uint32_t LZ4_DBG_Q_HIGH = 1u << 15, LZ4_DBG_Q_MAX = 1u << 31; // quality bits of `dbg` (zstd settings, lthip_launch_lz_sequences)

// slot of a private table of TAB entries for the (multiplied) hash `prod`: the upper 16 bits of prod times TAB, a 24-bit multiply and a
// shift (TAB < 2^16).  (mulhi(prod, TAB), what the batch parser takes, is a quarter-rate 32-bit multiply -- another function of the same
// bits: the tables fill differently, ratios agree to the fourth digit.)
template <int TAB>
__device__ __forceinline__ uint32_t lz4_tab_slot(uint32_t prod)
{
    return __umul24(prod >> 16, (uint32_t)TAB) >> 16;
}

// the first nonzero byte of four XOR words (16: none) without a branch: as an if / else-if chain every level is an exec-mask region
// of its own, three scalar instructions each, and all levels are walked anyway as soon as one lane of the wave gets there
__device__ __forceinline__ uint32_t lz4_first_diff16(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3)
{
    const uint64_t lo = (uint64_t)x0 | ((uint64_t)x1 << 32), hi = (uint64_t)x2 | ((uint64_t)x3 << 32);
    const uint32_t nlo = (uint32_t)__builtin_ctzll(lo | (1ull << 63)) >> 3, nhi = 8u + ((uint32_t)__builtin_ctzll(hi | (1ull << 63)) >> 3);
    return lo ? nlo : (hi ? nhi : 16u);
}
// equal leading bytes (0..16) of the 16 bytes at LDS byte addresses qa and qb (any alignment): five aligned dwords per side
__device__ __forceinline__ uint32_t lds_cmp16(uint32_t qa, uint32_t qb)
{
    const uint32_t wa = qa >> 2, wb = qb >> 2, da = qa, db = qb; // (v_alignbyte_b32 takes the two low bits)
    uint32_t ra[4], rb[4];
    lds_run<4>(wa, ra);
    lds_run<4>(wb, rb);
    const uint32_t a0 = ra[0], a1 = ra[1], a2 = ra[2], a3 = ra[3], a4 = lds_dw(wa + 4u);
    const uint32_t b0 = rb[0], b1 = rb[1], b2 = rb[2], b3 = rb[3], b4 = lds_dw(wb + 4u);
    const uint32_t x0 = __builtin_amdgcn_alignbyte(a1, a0, da) ^ __builtin_amdgcn_alignbyte(b1, b0, db);
    const uint32_t x1 = __builtin_amdgcn_alignbyte(a2, a1, da) ^ __builtin_amdgcn_alignbyte(b2, b1, db);
    const uint32_t x2 = __builtin_amdgcn_alignbyte(a3, a2, da) ^ __builtin_amdgcn_alignbyte(b3, b2, db);
    const uint32_t x3 = __builtin_amdgcn_alignbyte(a4, a3, da) ^ __builtin_amdgcn_alignbyte(b4, b3, db);
    return lz4_first_diff16(x0, x1, x2, x3);
}

template <int TAB, int FMT, int SH>
__device__ __forceinline__ void lz4_lane_parse2(const uint32_t* sdata, uint32_t head /* incl. LZ4_LPAD */, uint16_t* tab, const uint32_t* shr,
                                                uint32_t sh_base, int lane, uint32_t my_start, uint32_t my_len, int32_t start_limit,
                                                uint32_t end_limit, uint32_t sub, uint8_t* __restrict__ out, uint64_t* __restrict__ zrecs,
                                                Lz4Seq& st, uint32_t dbg K5P_ARG, uint32_t lo_bound = 0u, uint32_t sh_shift = 32u - (uint32_t)SH,
                                                uint32_t sh_off = 0u, uint32_t not_private = 0xFFFFFFFFu, uint32_t far1 = 0xFFFFFFFFu,
                                                uint32_t far2 = 0xFFFFFFFFu, uint32_t hist = 0u, uint32_t far3 = 4u)
{
    // hist != 0: the window below position `hist` is HISTORY (k_lz4_pair_halves): the shared table's lower half holds, per key, its LATEST
    // position there (stored inverted, so that the table's minimum is the nearest one) -- a third candidate, asked last; a match into the
    // history must have far3 bytes

    // not_private: a position the PRIVATE table never offers (an unlinked half's first position: in the window's lower half that is
    // position 0, which the table cannot tell from "empty", so the upper half must not have it either -- what a half compresses to must
    // not depend on which slot of the window it was given)
    // lo_bound: candidates below this window position are not this unit's history (two unrelated half-groups share the window, see
    // k_lz4_lanes2); sh_shift / sh_off: the part of the shared table that is this half's
    static_assert(SH != 0, "the second formulation is the shared-table parser's");
    static_assert(LZ4_LANE_MAXREC == 8, "records are eight register pairs");
    constexpr bool PAD = true; // the window is the padded one (lds_dw)
    constexpr bool rev = true;
    const int sidx = 63 - lane; // my sub-unit (reverse mapping: the lowest position survives a same-instruction write conflict)
    const uint32_t unit_end = my_start + my_len;
    const uint32_t s0 = my_start + (uint32_t)sidx * sub;
    const uint32_t lend = s0 + sub < unit_end ? s0 + sub : unit_end;
    uint32_t p = s0, anchor = s0, nrec = 0, last_end = 0, nmiss = 0;
    // ("deep" -- every byte position probed and, where both tables' candidates verify, the longer match taken, round 4's first "high"
    // setting -- measured WORSE with the history halves than without on every synthetic kind, and a third slower: DESIGN_HISTORY.md)
    const bool q_max = FMT == 1 && (dbg & LZ4_DBG_Q_MAX) != 0u;
    constexpr uint32_t dense = 4u;
    // Round 5, ADAPTIVE miss stepping.  After a hit (and at a sub-unit's start) a lane steps `dense` single bytes before it probes
    // aligned dwords only -- history enters the tables at aligned dwords, so a probe at an unaligned position is what finds a repeat
    // whose distance is not a multiple of four.  Data made of aligned structures (records, tables, tokens: what compresses in an asset
    // store) never answers such a probe: on bench.py's compressible tree the one-byte steps were 19 ms of the match finder's 166 and
    // bought nothing (profiles/r05_lane_dense_sweep.txt: none of them 314 GB/s at ratio 2.011, four of them 288 at 2.000; on word-soup
    // text none of them costs 5 % of the ratio, tools/text_ratio_probe.py).  So the WAVE
    // keeps count: after LZ4_QUIET probe rounds without a single hit at an unaligned position the one-byte steps stop; the first such
    // hit -- the probe behind a match's end stands wherever the match ended -- brings them back.  Wave-uniform, from ballots: a function
    // of the unit's data alone.
    constexpr uint32_t quiet_rounds = LZ4_QUIET; // (the sweep: profiles/r05_adaptive_stepping.txt)
    // (the state: bit k of qhist = an unaligned hit k probe rounds ago; bit 0 also stands for the unit's start)
    uint32_t qhist = 1u;
    bool dense_now = true;
    // lanes that must hold a hit before the wave turns to the extension: 4 (round 4, VALU bound: 2 GiB mixed 4.25 ms at 8, 4.12 at 4,
    // 4.16 / 4.37 / 4.76 at 16 / 32 / 48; tokens 5.97 / 5.93 / 6.03 / 6.80 / 7.78 -- waiting lanes are idle lanes)
    // (round 5, with the probe round at half its instructions: mixed 147.2 / 146.2 / 145.6 / 145.0 / 145.4 / 148.4 ms of match finder per
    // 64 GiB at 4 / 6 / 8 / 12 / 16 / 24, tokens 165.8 / 163.4 / 162.0 / 160.5 / 161.3 / 169.5: 12)
    constexpr uint32_t wait_for = 12u;
    uint32_t rsl[8], roff[8]; // records: start | length << 16, offset
#pragma unroll
    for (int k = 0; k < 8; ++k)
        rsl[k] = roff[k] = 0u;
    uint32_t cand = 0u;
    // The loop's conditions, one compare each (a ballot of a compare IS the compare; a ballot of a combination of conditions costs a
    // select and a second compare -- and the kernel is bound by the number of vector instructions it issues): a lane probes while
    // p < plim (the end of its sub-unit, the unit's last start; 0 once its records are full), and a hit that waits for its extension
    // sets p's top bit -- which also takes the lane out of p < plim.
    constexpr uint32_t PEND = 0x80000000u;
    const uint32_t headm1 = head - 1u;
    const uint32_t stop0 = start_limit < 0 ? 0u : ((uint32_t)start_limit + 1u < lend ? (uint32_t)start_limit + 1u : lend);
    uint32_t plim = stop0;
    for (;;)
    {
        // ---- probe rounds, until enough hits wait (or nobody can probe any more) ----
        uint64_t pm = 0ull;
        for (;;)
        {
            const bool act = p < plim;
            const uint64_t am = __builtin_amdgcn_ballot_w64(act);
            if (am == 0ull)
                break;
            const uint32_t x = p + head; // (the LDS byte address of position p)
            const uint64_t unm = __builtin_amdgcn_ballot_w64((x & 3u) != 0u); // lanes that stand at an unaligned position
            if (am)
            {
                if (act)
                {
                    // the four bytes at p: two aligned dwords, read where they are needed (round 4 kept the lane's next dwords in a register
                    // window that slid with p to save this round trip; since the kernel is bound by the vector instructions it issues, the
                    // window's bookkeeping -- reload after every jump, shift at every crossing, and the copies the three versions of
                    // every register cost at the loop's joins -- was 20 of a probe round's 110 instructions, the round trip is hidden)
                    uint32_t d2[2];
                    lds_run<2>(x >> 2, d2);
                    const uint32_t v = __builtin_amdgcn_alignbyte(d2[1], d2[0], x);
                    const uint32_t prod = v * 2654435761u;
                    const uint32_t h = lz4_tab_slot<TAB>(prod);
                    uint32_t c = tab[h];
                    const uint32_t c2 = shr[(prod >> sh_shift) + sh_off] - sh_base; // (another group's entry: far above any position)
                    tab[h] = (uint16_t)p;
                    if (q_max) // "max": the slot is read again after the step's inserts (entries of lanes in phase)
                    {
                        uint32_t hr = h;
                        asm volatile("" : "+v"(hr));
                        const uint32_t fresh = tab[hr];
                        if (fresh < p)
                            c = fresh;
                    }
                    // both candidates' bytes in one round trip (an invalid one reads my own position and is masked)
                    const bool v1 = c < p && c >= lo_bound && c != not_private, v2 = c2 < p && c2 >= lo_bound;
                    const uint32_t r1 = lds_read32x<PAD>(sdata, (v1 ? c : p) + head);
                    const uint32_t r2 = lds_read32x<PAD>(sdata, (v2 ? c2 : p) + head);
                    const bool h1 = v1 && r1 == v, h2 = v2 && r2 == v;
                    bool h3 = false;
                    uint32_t c3 = 0u;
                    if (FMT == 1 && hist)
                    {
                        const uint32_t e3 = shr[prod >> sh_shift] - sh_base; // (another item's entry: above 0xFFFF)
                        c3 = 0xFFFFu - e3;
                        const bool v3 = e3 <= 0xFFFFu;
                        h3 = v3 && lds_read32x<PAD>(sdata, (v3 ? c3 : p) + head) == v;
                    }
                    if (h1 || h2 || h3)
                    {
                        p |= PEND;
                        cand = h1 ? c : (h2 ? c2 : c3); // the private table's (the nearest one) first, the history's last
                    }
                    else
                    {
                        p = ((dense_now && nmiss < dense) ? x : (x | 3u)) - headm1;
                        ++nmiss;
                    }
                }
            }
            K5P(3);
            K5P_COUNT(10, 1);
            pm = __builtin_amdgcn_ballot_w64((int32_t)p < 0);
            {
                // (scalar: the hits of this round are the waiting lanes that probed)
                const uint64_t t = unm & pm & am;
                uint32_t bit; // t != 0 as 0 / 1 (written out: the compiler takes the truth value through a vector register)
                asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, 1, 0" : "=s"(bit) : "s"(t) : "scc");
                qhist = (qhist << 1) | bit;
                dense_now = (qhist & ((1u << quiet_rounds) - 1u)) != 0u;
            }
            if ((uint32_t)__builtin_popcountll(pm) >= wait_for)
                break; // (fewer: somebody may still probe -- let the hits pile up)
        }
        pm = __builtin_amdgcn_ballot_w64((int32_t)p < 0);
        if (pm == 0ull)
            break; // nobody probes, nobody waits: the unit is parsed
        bool ok = (int32_t)p < 0;
        p &= ~PEND;
        K5P_COUNT(11, 1);
        K5P_COUNT(12, (unsigned)__builtin_popcountll(pm));
        // ---- one round trip: 8 bytes backwards and the first 16 bytes forwards of every hit ----
        uint32_t mlen = 0, nbk = 0;
        bool grow = false;
        const uint32_t maxlen = ok ? end_limit - p : 0u; // p <= start_limit: at least 4
        if (ok)
        {
            const uint32_t qo = p + head - 8u, qc = cand + head - 8u;
            const uint32_t bo = qo >> 2, bc = qc >> 2, dlo = qo, dlc = qc; // (v_alignbyte_b32 takes the two low bits)
            uint32_t Do[8], Dc[8];
            lds_run<4>(bo, Do);
            lds_run<4>(bo + 4u, Do + 4);
            lds_run<4>(bc, Dc);
            lds_run<4>(bc + 4u, Dc + 4);
            uint32_t X[7];
#pragma unroll
            for (int k = 0; k < 7; ++k)
                X[k] = __builtin_amdgcn_alignbyte(Do[k + 1], Do[k], dlo) ^ __builtin_amdgcn_alignbyte(Dc[k + 1], Dc[k], dlc);
            const uint32_t add = lz4_first_diff16(X[3], X[4], X[5], X[6]); // bytes p + 4 .. p + 20
            mlen = 4u + add;
            grow = add == 16u;
            if (mlen >= maxlen)
            {
                mlen = maxlen;
                grow = false;
            }
            {
                // (unconditional: the distance to the anchor bounds it -- 0 at the anchor --, a candidate too close to the window's
                // lower bound takes none)
                const uint64_t bw = ((uint64_t)X[1] << 32) | (uint64_t)X[0];
                nbk = (uint32_t)__builtin_clzll(bw | 1ull) >> 3;
                nbk = bw ? nbk : 8u;
                nbk = nbk < p - anchor ? nbk : p - anchor;
                nbk = cand >= lo_bound + 8u ? nbk : 0u;
            }
        }
        // ---- matches of 20 bytes and more: one more 16-byte round of their own (at most 36 bytes), then the whole wave ----
        if (grow)
        {
            const uint32_t add = lds_cmp16(p + mlen + head, cand + mlen + head);
            mlen += add;
            if (add != 16u)
                grow = false;
            if (mlen >= maxlen)
            {
                mlen = maxlen;
                grow = false;
            }
        }
        uint64_t longs = __builtin_amdgcn_ballot_w64(grow);
        K5P(4);
        while (longs)
        {
            K5P_COUNT(13, 1);
            const int f = rev ? 63 - __builtin_clzll(longs) : __builtin_ctzll(longs);
            longs &= ~(1ull << f);
            const uint32_t pf = __builtin_amdgcn_readlane(p, f), cf = __builtin_amdgcn_readlane(cand, f);
            uint32_t ml = __builtin_amdgcn_readlane(mlen, f);
            for (;;)
            {
                const uint32_t i = pf + ml + 4u * (uint32_t)lane;
                uint32_t cnt = 0; // equal bytes of my four, as far as the unit goes
                if (i < end_limit)
                {
                    const uint32_t x = lds_read32x<PAD>(sdata, i + head) ^ lds_read32x<PAD>(sdata, cf + ml + 4u * (uint32_t)lane + head);
                    const uint32_t lim = end_limit - i < 4u ? end_limit - i : 4u;
                    cnt = x ? (uint32_t)__builtin_ctz(x) >> 3 : 4u;
                    cnt = cnt < lim ? cnt : lim;
                }
                const uint64_t diff = __builtin_amdgcn_ballot_w64(cnt < 4u);
                if (diff)
                {
                    const int g = __builtin_ctzll(diff);
                    ml += 4u * (uint32_t)g + __builtin_amdgcn_readlane(cnt, g);
                    break;
                }
                ml += 256u;
            }
            if (lane == f)
                mlen = ml;
            const uint32_t cov = pf + ml;
            const bool cv = p - (pf + 1u) < ml - 1u; // pf < p < cov, one compare (lane f itself stands at pf; waiting lanes' p carries no flag here)
            if (cv)
            {
                p = cov;
                anchor = anchor > cov ? anchor : cov;
                ok = false;
            }
            longs &= ~__builtin_amdgcn_ballot_w64(cv);
        }
        // the zstd flavour prices a match by its distance (the offset's bits are written out): four or five bytes from far away cost more
        // than the literals they replace -- such a hit counts as a miss (T1, T2: LTHIP_LZ4_FAR, measured in profiles/r04_zstd_ratio_table.txt)
        if (FMT == 1 && ok && mlen + nbk < (cand < hist ? far3 : 4u + (p - cand >= far1 ? 1u : 0u) + (p - cand >= far2 ? 1u : 0u)))
        {
            ok = false;
            p += 1u;
            ++nmiss;
        }
        else if (ok)
        {
            const uint32_t s = p - nbk, len = mlen + nbk;
            const uint32_t sl = s | (len << 16), of = p - cand;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (nrec == (uint32_t)k)
                {
                    rsl[k] = sl;
                    roff[k] = of;
                }
            ++nrec;
            if (nrec == LZ4_LANE_MAXREC)
                plim = 0u;
            p = s + len;
            anchor = p;
            last_end = p;
            nmiss = 0;
        }
        // (a waiting hit is either recorded or covered: nothing else to do)
        K5P(5);
    }

    // ---- what earlier sub-units' matches cover is dropped: exclusive prefix maximum of the match ends, in sub-unit order ----
    static_assert(rev, "the scans below run in lane order from the top");
    const uint32_t incl = lane_suffix_scan<true>(last_end, lane);
    const uint32_t cover = lane_from_sub_before(incl);
    uint32_t k0 = 0; // my first record that starts at or after the cover (starts ascend)
#pragma unroll
    for (int k = 0; k < 8; ++k)
        k0 += ((uint32_t)k < nrec && (rsl[k] & 0xFFFFu) < cover) ? 1u : 0u;
    const bool have = k0 < nrec;
    uint32_t first_start_v = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((uint32_t)k == k0)
            first_start_v = rsl[k] & 0xFFFFu;
    if (!have)
        first_start_v = 0u;
    // previous kept end = where the literals of my first kept sequence begin
    const uint32_t kincl = lane_suffix_scan<true>(have ? last_end : 0u, lane);
    uint32_t prev0 = lane_from_sub_before(kincl);
    prev0 = prev0 > my_start ? prev0 : my_start;
    // sizes
    const uint32_t cnt = have ? nrec - k0 : 0u;
    uint32_t bytes = 0, nlit = 0;
    {
        uint32_t prev = prev0;
#pragma unroll
        for (int k = 0; k < 8; ++k) // (a branch per slot on purpose: the last slots are rarely anybody's, and then the whole wave skips them)
        {
            const bool on = (uint32_t)k - k0 < cnt;
            const uint32_t s = rsl[k] & 0xFFFFu, len = rsl[k] >> 16;
            const uint32_t lit = s - prev;
            if (on)
            {
                bytes += 3u + lz4_len_bytes16(lit) + lit + lz4_len_bytes16(len - 4u);
                nlit += lit;
                prev = s + len;
            }
        }
    }
    const uint32_t a_incl = lane_suffix_scan<false>(FMT == 1 ? nlit : bytes, lane);
    const uint32_t c_incl = FMT == 1 ? lane_suffix_scan<false>(cnt, lane) : 0u;
    const uint32_t a_total = (uint32_t)__builtin_amdgcn_readlane((int)a_incl, 0); // (the last sub-unit is lane 0's)
    uint32_t o_pos = a_incl - (FMT == 1 ? nlit : bytes);
    uint32_t q_pos = FMT == 1 ? c_incl - cnt : 0u;
    const uint32_t last_kept_end = (uint32_t)__builtin_amdgcn_readlane((int)kincl, 0);

    K5P(6);
    // ---- emission: every lane writes its own sequences; literal runs above 16 bytes are copied by the whole wave ----
    {
        uint32_t prev = prev0;
        const uint64_t anyrec = __builtin_amdgcn_ballot_w64(cnt != 0u);
#pragma unroll
        for (int k = 0; k < 8; ++k)
        {
            const bool on = (uint32_t)k - k0 < cnt; // k0 <= k < nrec, one compare (cnt = nrec - k0, or 0)
            if (anyrec == 0ull || __builtin_amdgcn_ballot_w64(on) == 0ull)
                continue;
            uint32_t lit = 0, lit_src = 0, lit_dst = 0;
            if (on)
            {
                const uint32_t s = rsl[k] & 0xFFFFu, len = rsl[k] >> 16, off = roff[k];
                lit = s - prev;
                lit_src = prev;
                if constexpr (FMT == 1)
                {
                    lit_dst = o_pos;
                    zrecs[q_pos] = (uint64_t)lit | ((uint64_t)len << 16) | ((uint64_t)off << 32);
                    ++q_pos;
                    o_pos += lit;
                }
                else
                {
                    uint8_t* o = out + o_pos;
                    const uint32_t mcode = len - 4u;
                    o[0] = (uint8_t)(((lit < 15u ? lit : 15u) << 4) | (mcode < 15u ? mcode : 15u));
                    uint32_t idx = 1u;
                    if (lit >= 15u)
                    {
                        uint32_t rem = lit - 15u;
                        for (; rem >= 255u; rem -= 255u)
                            o[idx++] = 255;
                        o[idx++] = (uint8_t)rem;
                    }
                    lit_dst = o_pos + idx;
                    idx += lit;
                    o[idx] = (uint8_t)off;
                    o[idx + 1u] = (uint8_t)(off >> 8);
                    idx += 2u;
                    if (mcode >= 15u)
                    {
                        uint32_t rem = mcode - 15u;
                        for (; rem >= 255u; rem -= 255u)
                            o[idx++] = 255;
                        o[idx++] = (uint8_t)rem;
                    }
                    o_pos += idx;
                }
                prev = s + len;
                if (lit <= 16u)
                {
                    // four bytes per store where four are left (the destination has any alignment: global memory takes unaligned
                    // dwords), single bytes for the rest -- never a byte beyond the run: the next byte is another lane's
                    typedef uint32_t u32_a1 __attribute__((aligned(1)));
                    uint8_t* o = out + lit_dst;
                    uint32_t j = 0;
                    for (; j + 4u <= lit; j += 4u)
                        *reinterpret_cast<u32_a1*>(o + j) = lds_read32x<PAD>(sdata, lit_src + j + head);
                    for (; j < lit; ++j)
                        o[j] = (uint8_t)lds_byte<PAD>(sdata, lit_src + j + head);
                }
            }
            uint64_t big = __builtin_amdgcn_ballot_w64(lit > 16u); // (lit is 0 where the lane has no k-th sequence)
            while (big)
            {
                const int f = __builtin_ctzll(big);
                big &= big - 1ull;
                wave_copy_lds_to_global<PAD>(out + __builtin_amdgcn_readlane(lit_dst, f), sdata, __builtin_amdgcn_readlane(lit_src, f) + head,
                                        __builtin_amdgcn_readlane(lit, f), lane);
            }
        }
    }
    K5P(7);
    // ---- the unit's result, as the batch parser leaves it ----
    const uint64_t hm = __builtin_amdgcn_ballot_w64(have);
    st.have_first = hm != 0ull;
    st.anchor = hm ? last_kept_end : my_start;
    if constexpr (FMT == 1)
    {
        st.op = a_total; // literal bytes so far
        st.nseq = (uint32_t)__builtin_amdgcn_readlane((int)c_incl, 0);
    }
    else
    {
        st.op = a_total;
        if (hm)
        {
            const int f = 63 - __builtin_clzll(hm); // the lane of the first sub-unit with a sequence
            const uint32_t first_start = __builtin_amdgcn_readlane(first_start_v, f);
            st.first_lit = first_start - my_start;
            st.first_hdr = 1u + lz4_len_bytes(st.first_lit);
        }
    }
}

