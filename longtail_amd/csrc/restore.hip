// restore.hip -- the restore session (include/longtail_hip.h, "the restore session"): stored-block images in HBM back into the assets of
// a version, the device side of Longtail_WriteVersion (src/longtail.c:6471-6573; BuildAssetWriteList :6021, WriteAssetsFromBlock :5700)
// and DecompressBlock (compressblockstore.c:271-338).
//
//   create   the host expands the VersionIndex into OCCURRENCES (chunk hash, destination, length) -- prefix arithmetic over
//            m_AssetChunkIndexes and m_ChunkSizes -- and the StoreIndex into per-chunk (block, offset in block).  The device resolves:
//            the StoreIndex's chunk hashes go into an lthip_seen, lthip_seen_find gives every occurrence the position of its chunk,
//            k_restore_resolve checks the size and counts occurrences per block, an exclusive scan gives every block its first entry,
//            k_restore_fill places (offset in block, length, destination) block-major.  The block_count + 1 firsts come back once.
//   windows  (lthip_restore_create_windows, restore_windows.h) the occurrences are those of byte windows of assets, each CLIPPED to its
//            window: next to the chunk's full length it carries `skip` bytes into the chunk and `clip` bytes to write.  k_restore_resolve
//            still compares the full length with the StoreIndex's size and counts `clip` bytes; k_restore_fill places (offset in block +
//            skip, clip, destination).  A clipped occurrence is an ordinary entry: check, decode, verify and scatter do not know of it.
//            The sessions of whole assets are the same routine with one window per selected asset and no skip / clip tables at all.
//   blocks   k_restore_check_images (a wave per image, against the device copy of the StoreIndex) -> the decoders into 64-byte slots of
//            the caller's scratch -> k_restore_ranges (the decoders' verdict into the block's status word; with verify the (offset,
//            length) of every chunk) -> lthip_hash_ranges_by_id -> k_restore_compare -> k_restore_scatter over the call's entries.
//            Nothing is allocated and nothing is waited for: the session's tables were sized by create.
//   base     (lthip_restore_create_from_base) a version that lies restored in HBM is a second source.  The host expands it as it expands
//            the target: per distinct chunk the offset of its first occurrence in a resident asset.  Its chunk hashes go into a second
//            lthip_seen; k_restore_resolve gives an occurrence to the base when the base holds its hash with the same size at a resident
//            offset, and to the StoreIndex otherwise.  Base-fed occurrences are compacted in OCCURRENCE order (a scan over flags) into
//            (source offset, destination, length, base chunk); the base chunks that feed something are listed for verify.  All counts
//            come back with the plan's one read-back.
//   carry    k_restore_carry_bounds flags every entry that does not continue the one before it in source AND destination (with verify:
//            after the listed base chunks were hashed where they lie and compared, k_restore_carry_compare; an entry of a chunk that
//            differs is a boundary of its own and gets no pieces) -> scan -> k_restore_carry_runs: a boundary that starts a run finds
//            the next boundary by bisection of the scan and writes {source, destination, length} and the run's pieces into its slot ->
//            scan -> k_raw_copy (k_gather.hip).  An unchanged asset is one run.
//   in place (lthip_restore_carry_in_place) the base and the target share one buffer.  The same runs; k_restore_in_place_classify drops
//            the runs whose source is their destination (kept: nothing is queued) and gives every other run a 16-byte aligned slot in the
//            caller's scratch -> scans -> k_restore_in_place_slots -> k_raw_copy twice: every moved run buffer -> scratch, then scratch ->
//            buffer.  All reads come before all writes, so runs may overlap each other in any way.  How many entries move, and their bytes,
//            is counted by k_restore_fill and comes back with the plan's one read-back: the scratch bound is host arithmetic.
// The scatter and a decoder's second pass cost one more read and write of the output than decoding into place would: about a tenth on top
// of the bare decoder calls (profiles/restore_rate.json).
#include "lthip_internal.h"
#include "restore_layout.h"
#include "restore_parse.h"
#include "restore_windows.h"
#include "store_layout.h"
#include "version_diff.h"

#include <new>
#include <unordered_map>

namespace
{

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
constexpr int RT = 256;
constexpr uint32_t NONE = 0xFFFFFFFFu;

// one delivered, needed block of a lthip_restore_blocks call
struct RItem
{
    uint64_t image;  // where its image starts in d_images
    uint64_t src;    // device address of its chunks' bytes: the image's payload (raw block) or its scratch slot
    uint32_t size;   // bytes of the image
    uint32_t block;  // its index in the StoreIndex
    uint32_t raw;    // the sum of its chunk sizes
    uint32_t efirst; // its first entry among the call's entries ...
    uint32_t ebase;  // ... and in the plan
    uint32_t vfirst; // its first chunk among the call's verify ranges
};

// ---- plan ----
// what the plan kernels know of the base (all null without one): per occurrence its position among the base's chunks (lthip_seen_find),
// per base chunk its size and the offset of its first resident occurrence (NOWHERE: none)
constexpr uint64_t NOWHERE = ~0ull;
struct BasePlan
{
    const uint32_t* opos;
    const uint32_t* size;
    const uint64_t* off;
};
__device__ __forceinline__ bool base_feeds(const BasePlan& bp, uint32_t i, uint32_t len, uint32_t* q)
{
    if (!bp.opos)
        return false;
    *q = bp.opos[i];
    return *q != NONE && bp.size[*q] == len && bp.off[*q] != NOWHERE;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1)
        v += __shfl_xor(v, o, 64);
    return v;
}

// counters: [0] occurrences neither source resolves, [5] bytes the base feeds ([8], [9]: k_restore_fill)
// (oclip: the bytes a clipped occurrence writes, null when every occurrence is its whole chunk)
__global__ void k_restore_resolve(uint32_t n, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ olen,
                                  const uint32_t* __restrict__ oclip, const uint32_t* __restrict__ csize, const uint32_t* __restrict__ cblock,
                                  uint32_t* __restrict__ hist, unsigned long long* __restrict__ bbytes, unsigned long long* counters,
                                  BasePlan bp, uint32_t* __restrict__ oflag, uint32_t* __restrict__ bfeed, uint32_t* __restrict__ bmark)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    unsigned long long fed = 0;
    if (i < n)
    {
        const uint32_t len = olen[i];
        uint32_t q = NONE;
        if (base_feeds(bp, i, len, &q)) // the base wins when both hold the chunk
        {
            oflag[i] = 1u;
            atomicAdd(&bfeed[q], 1u);
            bmark[q] = 1u;
            fed = len;
        }
        else
        {
            if (oflag)
                oflag[i] = 0u;
            const uint32_t p = pos[i];
            const uint32_t b = p == NONE ? NONE : cblock[p];
            if (b == NONE || csize[p] != len)
                miss = true;
            else
            {
                atomicAdd(&hist[b], 1u);
                atomicAdd(&bbytes[b], (unsigned long long)(oclip ? oclip[i] : len));
            }
        }
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(miss);
    if (m && (threadIdx.x & 63) == 0)
        atomicAdd(counters, (unsigned long long)__builtin_popcountll(m));
    if (bp.opos)
    {
        fed = wave_sum(fed);
        if (fed && (threadIdx.x & 63) == 0)
            atomicAdd(counters + 5, fed);
    }
}

// the order of a block's entries is whatever the atomics give; the output does not depend on it.  The base's entries keep the order of
// the occurrences (ofirst: the scan of the flags): that order is what makes runs.
__global__ void k_restore_fill(uint32_t n, const uint32_t* __restrict__ pos, const uint32_t* __restrict__ olen, const uint32_t* __restrict__ oskip,
                               const uint32_t* __restrict__ oclip, const uint64_t* __restrict__ odst, const uint32_t* __restrict__ csize,
                               const uint32_t* __restrict__ cblock, const uint32_t* __restrict__ coff,
                               const uint32_t* __restrict__ firsts, uint32_t* __restrict__ cursor, uint4* __restrict__ entries, BasePlan bp,
                               const uint32_t* __restrict__ ofirst, uint64_t* __restrict__ ksrc, uint64_t* __restrict__ kdst,
                               uint32_t* __restrict__ klen, uint32_t* __restrict__ kchunk, unsigned long long* counters)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long moved = 0; // bytes of a base-fed entry whose source offset is not its destination (counters[8], [9]: in place)
    bool is_moved = false;
    if (i < n)
    {
        const uint32_t len = olen[i];
        const uint64_t d = odst[i];
        uint32_t q = NONE;
        if (base_feeds(bp, i, len, &q))
        {
            const uint32_t k = ofirst[i];
            const uint64_t src = bp.off[q];
            ksrc[k] = src;
            kdst[k] = d;
            klen[k] = len;
            kchunk[k] = q;
            is_moved = src != d;
            moved = is_moved ? len : 0u;
        }
        else
        {
            const uint32_t p = pos[i];
            const uint32_t b = p == NONE ? NONE : cblock[p];
            if (b != NONE && csize[p] == len)
            {
                const uint32_t slot = firsts[b] + atomicAdd(&cursor[b], 1u);
                // (skip + clip <= len == csize[p]: the entry stays inside its chunk, and the block's raw size is below 2^32)
                const uint32_t skip = oskip ? oskip[i] : 0u, clip = oclip ? oclip[i] : len;
                entries[slot] = make_uint4(coff[p] + skip, clip, (uint32_t)d, (uint32_t)(d >> 32));
            }
        }
    }
    if (!bp.opos)
        return;
    const uint64_t m = __builtin_amdgcn_ballot_w64(is_moved);
    moved = wave_sum(moved);
    if (m && (threadIdx.x & 63) == 0)
    {
        atomicAdd(counters + 8, (unsigned long long)__builtin_popcountll(m));
        atomicAdd(counters + 9, moved);
    }
}

// the base chunks that feed something, in chunk order (mfirst: the scan of their marks): the ranges verify hashes, and their 1 KiB
// leaves summed (counters[6]: lthip_hash_ranges_by_id wants the total)
__global__ void k_restore_carry_marked(uint32_t n, const uint32_t* __restrict__ bmark, const uint32_t* __restrict__ mfirst,
                                       const uint32_t* __restrict__ bsize, const uint64_t* __restrict__ boff, uint64_t* __restrict__ voff,
                                       uint32_t* __restrict__ vlen, uint32_t* __restrict__ vchunk, unsigned long long* counters)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long leaves = 0;
    if (q < n && bmark[q])
    {
        const uint32_t k = mfirst[q], len = bsize[q];
        voff[k] = boff[q];
        vlen[k] = len;
        vchunk[k] = q;
        leaves = len ? ((unsigned long long)len + 1023u) >> 10 : 1u;
    }
    leaves = wave_sum(leaves);
    if (leaves && (threadIdx.x & 63) == 0)
        atomicAdd(counters + 6, leaves);
}

// ---- carry ----
// counters: [2] base chunks whose hash differed, [3] the occurrences they would have fed, [4] and their bytes
__global__ void k_restore_carry_compare(uint32_t n, const uint64_t* __restrict__ vhash, const uint32_t* __restrict__ vchunk,
                                        const uint64_t* __restrict__ bhash, const uint32_t* __restrict__ bsize,
                                        const uint32_t* __restrict__ bfeed, uint32_t* __restrict__ bbad, unsigned long long* counters)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t q = vchunk[k];
    const bool bad = vhash[k] != bhash[q];
    bbad[q] = bad ? 1u : 0u;
    if (bad)
    {
        atomicAdd(counters + 2, 1ull);
        atomicAdd(counters + 3, (unsigned long long)bfeed[q]);
        atomicAdd(counters + 4, (unsigned long long)bfeed[q] * bsize[q]);
    }
}

// bound[i] = 1: entry i does not continue entry i - 1 -- it starts a run, or (bbad, verify) it is left out and breaks one
__global__ void k_restore_carry_bounds(uint32_t n, const uint64_t* __restrict__ ksrc, const uint64_t* __restrict__ kdst,
                                       const uint32_t* __restrict__ klen, const uint32_t* __restrict__ kchunk, const uint32_t* __restrict__ bbad,
                                       uint32_t* __restrict__ bound)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    bool b = i == 0 || (bbad && (bbad[kchunk[i]] || bbad[kchunk[i - 1]]));
    if (!b)
    {
        const uint64_t len = klen[i - 1];
        b = ksrc[i] != ksrc[i - 1] + len || kdst[i] != kdst[i - 1] + len;
    }
    bound[i] = b ? 1u : 0u;
}

// rank = the exclusive scan of bound (n + 1 entries).  A boundary that starts a run ends it before the next boundary: the first j > i
// with rank[j + 1] > rank[i] + 1, found by bisection (rank is monotone), or the end of the list.  The entries of a run follow each other
// in the destination, so its length is the end of its last entry - its start.
__global__ void k_restore_carry_runs(uint32_t n, const uint64_t* __restrict__ ksrc, const uint64_t* __restrict__ kdst,
                                     const uint32_t* __restrict__ klen, const uint32_t* __restrict__ kchunk, const uint32_t* __restrict__ bbad,
                                     const uint32_t* __restrict__ bound, const uint32_t* __restrict__ rank, uint64_t* __restrict__ run_src,
                                     uint64_t* __restrict__ run_dst, uint64_t* __restrict__ run_len, uint32_t* __restrict__ pieces)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t np = 0;
    if (bound[i] && !(bbad && bbad[kchunk[i]]))
    {
        const uint32_t r = rank[i] + 1u; // boundaries up to and including i
        uint32_t lo = i, hi = n;         // rank[lo + 1] == r (no boundary in (i, lo]); hi == n or rank[hi + 1] > r
        while (hi - lo > 1)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (rank[mid + 1] > r)
                hi = mid;
            else
                lo = mid;
        }
        const uint64_t d = kdst[i], len = kdst[lo] + klen[lo] - d;
        run_src[i] = ksrc[i];
        run_dst[i] = d;
        run_len[i] = len;
        np = lthip_raw_pieces(d, len);
    }
    pieces[i] = np;
}

// ---- the carry in place: behind k_restore_carry_runs.  A run whose source is its destination is KEPT and loses its pieces (a run is all
// kept or all moved: the distance from source to destination is constant over it).  A moved run goes through the caller's scratch: it
// gets the 16-byte units of its slot there and the pieces of its way IN (a slot starts on a 16-byte boundary); `pieces` stays what its
// way back OUT needs. ----
__global__ void k_restore_in_place_classify(uint32_t n, const uint64_t* __restrict__ run_src, const uint64_t* __restrict__ run_dst,
                                            const uint64_t* __restrict__ run_len, uint32_t* __restrict__ pieces, uint32_t* __restrict__ pieces_in,
                                            uint32_t* __restrict__ units)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t in = 0, u = 0;
    if (pieces[i])
    {
        if (run_src[i] == run_dst[i])
            pieces[i] = 0u;
        else
        {
            const uint64_t len = run_len[i];
            in = lthip_raw_pieces(0, len);
            u = (uint32_t)((len + 15u) >> 4); // (the moved bytes and their padding stay below 2^36: lthip_restore_carry_in_place)
        }
    }
    pieces_in[i] = in;
    units[i] = u;
}

// first_unit = the exclusive scan of the units: where every run's slot starts in the scratch
__global__ void k_restore_in_place_slots(uint32_t n, const uint32_t* __restrict__ first_unit, uint64_t* __restrict__ run_slot)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        run_slot[i] = (uint64_t)first_unit[i] << 4;
}

// ---- a delivered image against the StoreIndex: one wave per image ----
__global__ __launch_bounds__(64) void k_restore_check_images(const RItem* __restrict__ items, uint32_t k, const uint8_t* __restrict__ images,
                                                             const uint64_t* __restrict__ bhash, const uint32_t* __restrict__ bcoff,
                                                             const uint32_t* __restrict__ bcnt, const uint32_t* __restrict__ btag,
                                                             const uint32_t* __restrict__ braw, uint32_t hash_identifier,
                                                             const uint64_t* __restrict__ chash, const uint32_t* __restrict__ csize,
                                                             uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x;
    if (i >= k)
        return;
    const uint32_t lane = threadIdx.x;
    const RItem it = items[i];
    const uint32_t b = it.block, n = bcnt[b], tag = btag[b], c0 = bcoff[b], raw = braw[b];
    const uint64_t hdr = 20ull + 12ull * n + (tag ? 8u : 0u);
    uint32_t st = 0;
    if ((uint64_t)it.size < hdr) // (nothing of it is read)
        st = LTHIP_RESTORE_BAD_HEADER;
    else
    {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(images + it.image); // 8-byte aligned by contract
        bool bad = false;
        if (lane == 0)
        {
            const uint64_t h = bhash[b];
            bad = w[0] != (uint32_t)h || w[1] != (uint32_t)(h >> 32) || w[2] != hash_identifier || w[3] != n || w[4] != tag;
            if (tag) // [raw size][compressed size] behind the BlockIndex
                bad = bad || w[5ull + 3ull * n] != raw || (uint64_t)w[6ull + 3ull * n] != (uint64_t)it.size - hdr;
        }
        for (uint32_t j = lane; j < n; j += 64)
        {
            const uint64_t h = chash[c0 + j];
            bad = bad || w[5ull + 2ull * j] != (uint32_t)h || w[6ull + 2ull * j] != (uint32_t)(h >> 32) || w[5ull + 2ull * n + j] != csize[c0 + j];
        }
        if (__builtin_amdgcn_ballot_w64(bad))
            st = LTHIP_RESTORE_BAD_HEADER;
        else if (!tag && (uint64_t)it.size != hdr + raw) // a raw image is its BlockIndex and its chunks, no more and no less
            st = LTHIP_RESTORE_BAD_PAYLOAD;
    }
    if (lane == 0)
        status[b] = st;
}

// ---- behind the decoders: their verdict into the status word; with verify, the byte range of every chunk of the good blocks (a bad
// block's chunks become empty ranges at offset 0: nothing of it is read) ----
__global__ __launch_bounds__(64) void k_restore_ranges(const RItem* __restrict__ items, uint32_t k, const uint32_t* __restrict__ outsz,
                                                       const uint32_t* __restrict__ bcoff, const uint32_t* __restrict__ bcnt,
                                                       const uint32_t* __restrict__ csize, const uint32_t* __restrict__ coff,
                                                       uint32_t* __restrict__ status, uint32_t verify, uint64_t base, uint64_t* __restrict__ voff,
                                                       uint32_t* __restrict__ vlen, uint32_t* __restrict__ vblock, uint32_t* __restrict__ vchunk)
{
    const uint32_t i = blockIdx.x;
    if (i >= k)
        return;
    const uint32_t lane = threadIdx.x;
    const RItem it = items[i];
    const uint32_t b = it.block;
    uint32_t st = status[b];
    if (!(st & LTHIP_RESTORE_BAD_HEADER) && outsz[i] != it.raw) // (the payload behind a wrong header is not judged)
        st |= LTHIP_RESTORE_BAD_PAYLOAD;
    if (lane == 0)
        status[b] = st;
    if (!verify)
        return;
    const uint32_t c0 = bcoff[b], n = bcnt[b];
    for (uint32_t j = lane; j < n; j += 64)
    {
        const uint32_t r = it.vfirst + j, c = c0 + j;
        voff[r] = st ? 0ull : it.src - base + coff[c];
        vlen[r] = st ? 0u : csize[c];
        vblock[r] = b;
        vchunk[r] = c;
    }
}

__global__ void k_restore_compare(uint32_t n, const uint64_t* __restrict__ vhash, const uint32_t* __restrict__ vblock,
                                  const uint32_t* __restrict__ vchunk, const uint64_t* __restrict__ chash, uint32_t* status,
                                  unsigned long long* mismatched)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n)
        return;
    const uint32_t b = vblock[r];
    // (the header and payload bits were final before this launch; only the chunk bit is set beside these reads)
    if (__hip_atomic_load(&status[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (LTHIP_RESTORE_BAD_HEADER | LTHIP_RESTORE_BAD_PAYLOAD))
        return;
    if (vhash[r] != chash[vchunk[r]])
    {
        atomicOr(&status[b], LTHIP_RESTORE_BAD_CHUNK);
        atomicAdd(mismatched, 1ull);
    }
}

// ---- the scatter: a workgroup per entry of the call's blocks, block-major.  The copy is k_gather_ranges' (k_gather.hip): the head up to
// the destination's 16-byte boundary and the tail by bytes, in between 16-byte stores of a source realigned from dwords with v_alignbit.
// The dwords loaded are those that hold a byte of the vector: q[0..3] always do (the source lies mis < 4 bytes into q[0]), q[4] is
// loaded only when mis != 0, and then it holds the vector's last mis bytes.  Source and destination sit at any byte positions. ----
__global__ __launch_bounds__(RT) void k_restore_scatter(const RItem* __restrict__ items, uint32_t k, const uint4* __restrict__ entries,
                                                        const uint32_t* __restrict__ status, const uint32_t* __restrict__ outsz,
                                                        uint32_t entry0, uint8_t* __restrict__ out)
{
    const uint32_t e = entry0 + blockIdx.x;
    uint32_t lo = 0, hi = k; // items[lo].efirst <= e < items[hi].efirst: the block that owns entry e (every item has entries)
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (items[mid].efirst <= e)
            lo = mid;
        else
            hi = mid;
    }
    const RItem it = items[lo];
    if (status[it.block] != 0u || outsz[lo] != it.raw) // no byte of a bad block reaches the output
        return;
    const uint4 en = entries[it.ebase + (e - it.efirst)];
    const int tid = threadIdx.x;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(it.src) + en.x;
    uint8_t* d = out + ((uint64_t)en.z | ((uint64_t)en.w << 32));
    uint32_t n = en.y;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)d & 15u)) & 15u);
    if (head > n)
        head = n;
    if ((uint32_t)tid < head)
        d[tid] = s[tid];
    d += head;
    s += head;
    n -= head;
    const uint32_t nvec = n >> 4;
    const uint32_t mis = (uint32_t)((uintptr_t)s & 3u);
    const uint32_t sh = mis * 8u;
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s - mis);
    for (uint32_t v = tid; v < nvec; v += RT)
    {
        const uint32_t* q = s4 + (size_t)v * 4u;
        const u32x4_a4 a = *reinterpret_cast<const u32x4_a4*>(q);
        const uint32_t x = mis ? q[4] : 0u;
        uint4 o;
        o.x = __builtin_amdgcn_alignbit(a.y, a.x, sh);
        o.y = __builtin_amdgcn_alignbit(a.z, a.y, sh);
        o.z = __builtin_amdgcn_alignbit(a.w, a.z, sh);
        o.w = __builtin_amdgcn_alignbit(x, a.w, sh);
        *reinterpret_cast<uint4*>(d + (size_t)v * 16u) = o;
    }
    const uint32_t done = nvec << 4;
    if ((uint32_t)tid < n - done)
        d[done + tid] = s[done + tid];
}

// host table -> device through the staging ring, in pieces, so that no staging slot grows to the size of an index
int upload(lthip_ctx* ctx, void* d_dst, const void* h_src, size_t bytes)
{
    constexpr size_t PIECE = 4u << 20;
    for (size_t o = 0; o < bytes; o += PIECE)
    {
        const int err = lthip_stage_upload(ctx, (uint8_t*)d_dst + o, (const uint8_t*)h_src + o, std::min(PIECE, bytes - o), ctx->stream);
        if (err)
            return err;
    }
    return 0;
}

// sub-allocation of one device allocation: sizes first (p == null), then the same calls again hand out the pieces
struct Carver
{
    uint8_t* p = nullptr;
    size_t at = 0;
    template <class T> void take(T** out, size_t count)
    {
        if (p)
            *out = reinterpret_cast<T*>(p + at);
        at += (count * sizeof(T) + 255u) & ~(size_t)255u;
    }
};

uint64_t round64(uint64_t x) { return (x + 63u) & ~(uint64_t)63u; }

} // namespace

struct lthip_restore
{
    lthip_ctx* ctx = nullptr;
    uint32_t verify = 0, hash_identifier = 0;
    uint32_t nb = 0, m = 0, nocc = 0, max_chunk = 0;
    uint64_t block_chunks = 0; // the blocks' chunk counts summed: m for an index whose blocks share no chunk position
    uint64_t assets_selected = 0, needed = 0, needed_delivered = 0, delivered_all = 0, unneeded = 0;
    bool finished = false;
    // the base: its distinct chunks, what of the plan it feeds (the read-back of create), whether carry has queued it
    bool has_base = false, carried = false;
    uint32_t nub = 0, ncarry = 0, nmarked = 0, base_max_chunk = 0;
    uint64_t out_bytes = 0, base_window = 0, carry_bytes = 0, carry_leaves = 0, moved_occ = 0, moved_bytes = 0;
    // in place: blocks calls that queued work (an in-place carry comes before them), the buffer an in-place carry was given
    bool blocks_queued = false, in_place = false;
    void* in_place_buf = nullptr;
    // the StoreIndex and the plan on the host
    std::vector<uint64_t> bhash, bbytes, bleaves;
    std::vector<uint32_t> bcnt, btag, braw, firsts, status;
    std::vector<uint8_t> delivered, in_call;
    std::unordered_map<uint64_t, uint32_t> block_of_hash;
    // the device side: one allocation for what lives as long as the session, one for what only the plan needs
    lthip_seen *seen = nullptr, *seen_base = nullptr;
    void *d_mem = nullptr, *d_tmp = nullptr;
    uint64_t *d_chash = nullptr, *d_bhash = nullptr, *d_voff = nullptr, *d_vhash = nullptr;
    uint32_t *d_csize = nullptr, *d_cblock = nullptr, *d_coff = nullptr, *d_bcoff = nullptr, *d_bcnt = nullptr, *d_btag = nullptr, *d_braw = nullptr,
             *d_status = nullptr, *d_firsts = nullptr, *d_outsz = nullptr, *d_vlen = nullptr, *d_vblock = nullptr, *d_vchunk = nullptr;
    uint4* d_entries = nullptr;
    RItem* d_items = nullptr;
    // [0] occurrences neither source resolves, [1] chunks of blocks whose hash differed, [2] base chunks whose hash differed, [3] the
    // occurrences those would have fed, [4] and their bytes, [5] bytes the base feeds, [6] 1 KiB leaves of the base chunks that feed,
    // [8] base-fed entries whose source offset is not their destination (moved: an update in place copies them) [9] and their bytes
    unsigned long long* d_counters = nullptr;
    // base-fed entries in occurrence order (room for every occurrence: how many the base feeds is known after the plan has run), per
    // base chunk {hash, size, offset in d_base, occurrences fed, hash differed}, and with verify the ranges of the chunks that feed
    uint64_t *d_ksrc = nullptr, *d_kdst = nullptr, *d_uhash = nullptr, *d_uoff = nullptr, *d_cvoff = nullptr, *d_cvhash = nullptr;
    uint32_t *d_klen = nullptr, *d_kchunk = nullptr, *d_usize = nullptr, *d_ufeed = nullptr, *d_ubad = nullptr, *d_cvlen = nullptr,
             *d_cvchunk = nullptr;
    // host tables of a lthip_restore_blocks call, kept for their capacity
    std::vector<RItem> items;
    std::vector<uint32_t> outsz, group[3], c_size, c_cap;
    std::vector<uint64_t> c_src, c_dst;

    bool is_needed(uint32_t b) const { return firsts[b + 1] != firsts[b]; }
    void carve(Carver& c, size_t items_cap)
    {
        c.take(&d_chash, m), c.take(&d_csize, m), c.take(&d_cblock, m), c.take(&d_coff, m);
        c.take(&d_bhash, nb), c.take(&d_bcoff, nb), c.take(&d_bcnt, nb), c.take(&d_btag, nb), c.take(&d_braw, nb), c.take(&d_status, nb);
        c.take(&d_firsts, (size_t)nb + 1), c.take(&d_entries, nocc), c.take(&d_items, items_cap), c.take(&d_outsz, items_cap), c.take(&d_counters, 10);
        if (verify)
            c.take(&d_voff, block_chunks), c.take(&d_vhash, block_chunks), c.take(&d_vlen, block_chunks), c.take(&d_vblock, block_chunks),
                c.take(&d_vchunk, block_chunks);
        if (has_base)
            c.take(&d_ksrc, nocc), c.take(&d_kdst, nocc), c.take(&d_klen, nocc), c.take(&d_kchunk, nocc), c.take(&d_uhash, nub),
                c.take(&d_uoff, nub), c.take(&d_usize, nub), c.take(&d_ufeed, nub), c.take(&d_ubad, nub);
        if (has_base && verify)
            c.take(&d_cvoff, nub), c.take(&d_cvhash, nub), c.take(&d_cvlen, nub), c.take(&d_cvchunk, nub);
    }
};

extern "C" int lthip_restore_layout(const void* version_index, size_t size, uint64_t align, uint64_t* asset_offsets, uint32_t* asset_count,
                                    uint64_t* total_bytes)
{
    if (!version_index)
        return EINVAL;
    restore_parse::VersionIndex v;
    int err = restore_parse::parse_version_index(version_index, size, &v);
    if (!err)
        err = restore_parse::layout(v, align, asset_offsets, total_bytes);
    if (!err && asset_count)
        *asset_count = v.asset_count;
    return err;
}

extern "C" void lthip_restore_destroy(lthip_restore* r)
{
    if (!r)
        return;
    (void)hipSetDevice(r->ctx->device);
    if (r->d_mem || r->d_tmp)
        (void)hipStreamSynchronize(r->ctx->stream);
    lthip_seen_destroy(r->seen);
    lthip_seen_destroy(r->seen_base);
    if (r->d_mem)
        (void)hipFree(r->d_mem);
    if (r->d_tmp)
        (void)hipFree(r->d_tmp);
    delete r;
}

// What a session writes: byte windows of assets (lthip_restore_create_windows), or whole assets at asset_offsets -- which become one
// window per selected asset once the VersionIndex has been read.
struct Wanted
{
    const char* who;
    const uint64_t* asset_offsets;
    bool by_window;
    uint64_t window_count;
    const restore_windows::Window* windows;
};

// `base` is optional: lthip_restore_create passes none, and then every step that serves it is skipped
static int restore_build(lthip_restore* r, const lthip_restore_config* cfg, const lthip_restore_base* base, const void* version_index,
                         size_t vi_size, const void* store_index, size_t si_size, const Wanted& wanted, uint64_t out_bytes)
{
    lthip_ctx* ctx = r->ctx;
    restore_parse::VersionIndex vi, bvi;
    restore_parse::StoreIndex si;
    if (restore_parse::parse_version_index(version_index, vi_size, &vi))
        return lthip_fail(ctx, EBADF, "lthip_restore_create", "malformed version index");
    if (restore_parse::parse_store_index(store_index, si_size, &si))
        return lthip_fail(ctx, EBADF, "lthip_restore_create", "malformed store index");
    if (si.chunk_count && si.hash_identifier != vi.hash_identifier)
        return lthip_fail(ctx, EINVAL, "lthip_restore_create", "the version index and the store index carry different hash identifiers");
    if (!wanted.by_window && vi.asset_count && !wanted.asset_offsets)
        return EINVAL;
    if (cfg)
    {
        if (cfg->struct_size < 8 || cfg->struct_size > 4096)
            return lthip_fail(ctx, EINVAL, "lthip_restore_create", "config->struct_size must be set to sizeof(lthip_restore_config)");
        r->verify = cfg->struct_size >= 12 && cfg->verify ? 1u : 0u;
    }
    r->hash_identifier = vi.hash_identifier;
    r->out_bytes = out_bytes;
    // ---- the base: per distinct chunk the offset of its first occurrence in a resident asset ----
    std::vector<uint64_t> uhash, uoff;
    std::vector<uint32_t> usize;
    if (base)
    {
        if (base->struct_size < sizeof(lthip_restore_base) || base->struct_size > 4096)
            return lthip_fail(ctx, EINVAL, "lthip_restore_create_from_base", "base->struct_size must be set to sizeof(lthip_restore_base)");
        if (restore_parse::parse_version_index(base->version_index, (size_t)base->version_index_size, &bvi))
            return lthip_fail(ctx, EBADF, "lthip_restore_create_from_base", "malformed version index of the base");
        if (bvi.hash_identifier != vi.hash_identifier)
            return lthip_fail(ctx, EINVAL, "lthip_restore_create_from_base", "the base and the target carry different hash identifiers");
        if (bvi.asset_count && !base->asset_offsets)
            return EINVAL;
        r->has_base = true;
        r->base_window = base->base_bytes;
        const uint32_t nub = r->nub = bvi.chunk_count;
        if (nub > 0x7FFFFFFFu)
            return lthip_fail(ctx, EINVAL, "lthip_restore_create_from_base", "more than 2^31 - 1 chunks in the base");
        uhash.resize(nub), usize.resize(nub), uoff.assign(nub, NOWHERE);
        for (uint32_t c = 0; c < nub; ++c)
        {
            uhash[c] = bvi.chunk_hashes[c];
            usize[c] = bvi.chunk_sizes[c];
            r->base_max_chunk = std::max(r->base_max_chunk, usize[c]);
        }
        for (uint64_t a = 0; a < bvi.asset_count; ++a)
        {
            const uint64_t off = base->asset_offsets[a], size = bvi.asset_sizes[a];
            if (off == restore_parse::SKIP || !size)
                continue;
            if (off > base->base_bytes || size > base->base_bytes - off)
                return lthip_fail(ctx, EINVAL, "lthip_restore_create_from_base", "a resident asset's window leaves the base");
            const uint64_t start = bvi.asset_chunk_index_starts[a], count = bvi.asset_chunk_counts[a];
            uint64_t at = off;
            for (uint64_t k = 0; k < count; ++k)
            {
                const uint32_t c = bvi.asset_chunk_indexes[start + k];
                if (uoff[c] == NOWHERE)
                    uoff[c] = at;
                at += usize[c];
            }
        }
    }
    // ---- occurrences: per window and chunk it touches (hash, full length, skip, clip, destination); a selected asset is one window of
    // all its bytes at its offset (a directory or an empty file: a window of no bytes, whatever its offset) ----
    restore_windows::Occurrences occ;
    {
        std::vector<restore_windows::Window> whole;
        if (!wanted.by_window)
            for (uint64_t a = 0; a < vi.asset_count; ++a)
            {
                const uint64_t off = wanted.asset_offsets[a], size = vi.asset_sizes[a];
                if (off != restore_parse::SKIP)
                    whole.push_back(restore_windows::Window{(uint32_t)a, 0u, 0u, size, size ? off : 0u});
            }
        const char* why = "";
        const int refused = wanted.by_window ? restore_windows::expand(vi, wanted.window_count, wanted.windows, out_bytes, &occ, &why)
                                             : restore_windows::expand(vi, whole.size(), whole.data(), out_bytes, &occ, &why);
        if (refused)
            return lthip_fail(ctx, refused, wanted.who, why);
    }
    r->assets_selected = occ.assets_selected;
    const std::vector<uint64_t>&ohash = occ.hash, &odst = occ.dst;
    const std::vector<uint32_t>& olen = occ.len;
    const bool clipped = !occ.clip.empty();
    // ---- the StoreIndex: per block its tables, per chunk position the block that holds it and where ----
    const uint32_t nb = r->nb = si.block_count, m = r->m = si.chunk_count;
    const uint32_t nocc = r->nocc = (uint32_t)ohash.size();
    if (m > 0x7FFFFFFFu)
        return lthip_fail(ctx, EINVAL, "lthip_restore_create", "more than 2^31 - 1 chunks in the store index");
    std::vector<uint64_t> chash(m);
    std::vector<uint32_t> csize(m), cblock(m, NONE), coff(m, 0u), bcoff(nb);
    for (uint32_t c = 0; c < m; ++c)
    {
        chash[c] = si.chunk_hashes[c];
        csize[c] = si.chunk_sizes[c];
        r->max_chunk = std::max(r->max_chunk, csize[c]);
    }
    r->bhash.resize(nb), r->bcnt.resize(nb), r->btag.resize(nb), r->braw.resize(nb), r->bleaves.resize(nb);
    for (uint32_t b = 0; b < nb; ++b)
    {
        r->bhash[b] = si.block_hashes[b];
        bcoff[b] = si.block_chunk_offsets[b];
        r->bcnt[b] = si.block_chunk_counts[b];
        r->btag[b] = si.block_tags[b];
        uint64_t off = 0, leaves = 0;
        for (uint32_t k = 0; k < r->bcnt[b]; ++k)
        {
            const uint32_t c = bcoff[b] + k;
            if (cblock[c] == NONE) // (blocks that share a chunk position: no writer produces them; the first block keeps it)
            {
                cblock[c] = b;
                coff[c] = (uint32_t)off;
            }
            off += csize[c];
            leaves += csize[c] ? ((uint64_t)csize[c] + 1023u) >> 10 : 1u;
        }
        r->braw[b] = (uint32_t)off; // (below 4 GiB: parse_store_index)
        r->block_chunks += r->bcnt[b];
        r->bleaves[b] = leaves;
        r->block_of_hash.emplace(r->bhash[b], b);
    }
    if (r->block_chunks > 0x7FFFFFFFull)
        return lthip_fail(ctx, EINVAL, "lthip_restore_create", "the store index's blocks list more than 2^31 - 1 chunks");
    r->delivered.assign(nb, 0), r->in_call.assign(nb, 0), r->status.assign(nb, 0u);
    r->firsts.assign((size_t)nb + 1, 0u), r->bbytes.assign(nb, 0ull);
    // ---- device memory: the session's, and the plan's temporaries ----
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    Carver size_of;
    r->carve(size_of, nb);
    LTHIP_CHECK(ctx, lthip_hip_malloc(&r->d_mem, size_of.at + 256));
    Carver place;
    place.p = (uint8_t*)r->d_mem;
    r->carve(place, nb);
    uint64_t *t_ohash = nullptr, *t_odst = nullptr;
    unsigned long long* t_bbytes = nullptr;
    uint32_t *t_olen = nullptr, *t_pos = nullptr, *t_hist = nullptr, *t_cursor = nullptr, *t_first = nullptr, *t_oskip = nullptr,
             *t_oclip = nullptr;
    uint32_t *t_bpos = nullptr, *t_oflag = nullptr, *t_ofirst = nullptr, *t_bfirst = nullptr, *t_bmark = nullptr, *t_mfirst = nullptr;
    const uint32_t nub = r->nub;
    for (int pass = 0; pass < 2; ++pass)
    {
        Carver c;
        c.p = (uint8_t*)r->d_tmp;
        c.take(&t_ohash, nocc), c.take(&t_odst, nocc), c.take(&t_bbytes, nb), c.take(&t_olen, nocc), c.take(&t_pos, nocc), c.take(&t_hist, nb),
            c.take(&t_cursor, nb), c.take(&t_first, m);
        if (clipped)
            c.take(&t_oskip, nocc), c.take(&t_oclip, nocc);
        if (base)
            c.take(&t_bpos, nocc), c.take(&t_oflag, nocc), c.take(&t_ofirst, (size_t)nocc + 1), c.take(&t_bfirst, nub), c.take(&t_bmark, nub),
                c.take(&t_mfirst, (size_t)nub + 1);
        if (pass == 0)
            LTHIP_CHECK(ctx, lthip_hip_malloc(&r->d_tmp, c.at + 256));
    }
    hipStream_t s = ctx->stream;
    int err;
    if ((err = upload(ctx, r->d_chash, chash.data(), (size_t)m * 8)) || (err = upload(ctx, r->d_csize, csize.data(), (size_t)m * 4)) ||
        (err = upload(ctx, r->d_cblock, cblock.data(), (size_t)m * 4)) || (err = upload(ctx, r->d_coff, coff.data(), (size_t)m * 4)) ||
        (err = upload(ctx, r->d_bhash, r->bhash.data(), (size_t)nb * 8)) || (err = upload(ctx, r->d_bcoff, bcoff.data(), (size_t)nb * 4)) ||
        (err = upload(ctx, r->d_bcnt, r->bcnt.data(), (size_t)nb * 4)) || (err = upload(ctx, r->d_btag, r->btag.data(), (size_t)nb * 4)) ||
        (err = upload(ctx, r->d_braw, r->braw.data(), (size_t)nb * 4)) || (err = upload(ctx, t_ohash, ohash.data(), (size_t)nocc * 8)) ||
        (err = upload(ctx, t_odst, odst.data(), (size_t)nocc * 8)) || (err = upload(ctx, t_olen, olen.data(), (size_t)nocc * 4)))
        return err;
    if (clipped &&
        ((err = upload(ctx, t_oskip, occ.skip.data(), (size_t)nocc * 4)) || (err = upload(ctx, t_oclip, occ.clip.data(), (size_t)nocc * 4))))
        return err;
    if (base && ((err = upload(ctx, r->d_uhash, uhash.data(), (size_t)nub * 8)) || (err = upload(ctx, r->d_uoff, uoff.data(), (size_t)nub * 8)) ||
                 (err = upload(ctx, r->d_usize, usize.data(), (size_t)nub * 4))))
        return err;
    if (base && nub)
    {
        LTHIP_CHECK(ctx, hipMemsetAsync(r->d_ufeed, 0, (size_t)nub * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(r->d_ubad, 0, (size_t)nub * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t_bmark, 0, (size_t)nub * 4, s));
    }
    LTHIP_CHECK(ctx, hipMemsetAsync(r->d_counters, 0, 80, s));
    if (nb)
    {
        LTHIP_CHECK(ctx, hipMemsetAsync(r->d_status, 0, (size_t)nb * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t_hist, 0, (size_t)nb * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t_cursor, 0, (size_t)nb * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t_bbytes, 0, (size_t)nb * 8, s));
    }
    // ---- the plan: hash -> position in the StoreIndex's chunk list, occurrences per block, firsts, entries block-major ----
    if ((err = lthip_seen_create(ctx, m, &r->seen)) || (err = lthip_seen_add(r->seen, m, r->d_chash, t_first, nullptr)))
        return err;
    // ... and, with a base, hash -> position among the base's chunks: an occurrence the base feeds is not resolved against the StoreIndex
    BasePlan bp = {nullptr, nullptr, nullptr};
    if (base)
    {
        if ((err = lthip_seen_create(ctx, nub, &r->seen_base)) || (err = lthip_seen_add(r->seen_base, nub, r->d_uhash, t_bfirst, nullptr)))
            return err;
        if (nocc && (err = lthip_seen_find(r->seen_base, nocc, t_ohash, t_bpos)))
            return err;
        bp = BasePlan{t_bpos, r->d_usize, r->d_uoff};
    }
    if (nocc)
    {
        if ((err = lthip_seen_find(r->seen, nocc, t_ohash, t_pos)))
            return err;
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_restore_resolve, dim3((nocc + 255u) / 256u), dim3(256), 0, s, nocc, (const uint32_t*)t_pos, (const uint32_t*)t_olen,
                           (const uint32_t*)t_oclip, (const uint32_t*)r->d_csize, (const uint32_t*)r->d_cblock, t_hist, t_bbytes, r->d_counters, bp,
                           t_oflag, r->d_ufeed, t_bmark);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if ((err = lthip_exclusive_scan_u32(ctx, t_hist, r->d_firsts, nb, nullptr, LTHIP_K_OTHER)))
        return err;
    if (base && ((err = lthip_exclusive_scan_u32(ctx, t_oflag, t_ofirst, nocc, nullptr, LTHIP_K_OTHER)) ||
                 (err = lthip_exclusive_scan_u32(ctx, t_bmark, t_mfirst, nub, nullptr, LTHIP_K_OTHER))))
        return err;
    if (nocc)
    {
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_restore_fill, dim3((nocc + 255u) / 256u), dim3(256), 0, s, nocc, (const uint32_t*)t_pos, (const uint32_t*)t_olen,
                           (const uint32_t*)t_oskip, (const uint32_t*)t_oclip, (const uint64_t*)t_odst, (const uint32_t*)r->d_csize,
                           (const uint32_t*)r->d_cblock, (const uint32_t*)r->d_coff, (const uint32_t*)r->d_firsts, t_cursor, r->d_entries, bp,
                           (const uint32_t*)t_ofirst, r->d_ksrc, r->d_kdst, r->d_klen, r->d_kchunk, r->d_counters);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if (base && r->verify && nub)
    {
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_restore_carry_marked, dim3((nub + 255u) / 256u), dim3(256), 0, s, nub, (const uint32_t*)t_bmark,
                           (const uint32_t*)t_mfirst, (const uint32_t*)r->d_usize, (const uint64_t*)r->d_uoff, r->d_cvoff, r->d_cvlen,
                           r->d_cvchunk, r->d_counters);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    // ---- the one read-back: the firsts (and the bytes per block, for the statistics), what did not resolve, what the base feeds ----
    unsigned long long counters[10] = {0};
    LTHIP_CHECK(ctx, hipMemcpyAsync(r->firsts.data(), r->d_firsts, ((size_t)nb + 1) * 4, hipMemcpyDeviceToHost, s));
    if (nb)
        LTHIP_CHECK(ctx, hipMemcpyAsync(r->bbytes.data(), t_bbytes, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
    LTHIP_CHECK(ctx, hipMemcpyAsync(counters, r->d_counters, sizeof counters, hipMemcpyDeviceToHost, s));
    if (base)
    {
        LTHIP_CHECK(ctx, hipMemcpyAsync(&r->ncarry, t_ofirst + nocc, 4, hipMemcpyDeviceToHost, s));
        LTHIP_CHECK(ctx, hipMemcpyAsync(&r->nmarked, t_mfirst + nub, 4, hipMemcpyDeviceToHost, s));
    }
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    if (counters[0])
        return lthip_fail(ctx, ENOENT, wanted.who,
                          base ? "a selected asset needs a chunk that neither the base nor the store index holds (or holds with another size)"
                               : "a selected asset or window needs a chunk the store index does not hold (or holds with another size)");
    r->carry_bytes = counters[5];
    r->carry_leaves = counters[6];
    r->moved_occ = counters[8];
    r->moved_bytes = counters[9];
    lthip_seen_destroy(r->seen_base);
    r->seen_base = nullptr;
    LTHIP_CHECK(ctx, hipFree(r->d_tmp));
    r->d_tmp = nullptr;
    for (uint32_t b = 0; b < nb; ++b)
        r->needed += r->is_needed(b);
    return 0;
}

static int restore_create(lthip_ctx* ctx, const lthip_restore_config* cfg, const lthip_restore_base* base, const void* version_index,
                          size_t vi_size, const void* store_index, size_t si_size, const Wanted& wanted, uint64_t out_bytes, lthip_restore** out)
{
    if (!ctx || !out || !version_index || !store_index)
        return EINVAL;
    *out = nullptr;
    lthip_restore* r = new (std::nothrow) lthip_restore();
    if (!r)
        return ENOMEM;
    r->ctx = ctx;
    int err;
    try
    {
        err = restore_build(r, cfg, base, version_index, vi_size, store_index, si_size, wanted, out_bytes);
    }
    catch (const std::bad_alloc&)
    {
        err = lthip_fail(ctx, ENOMEM, "lthip_restore_create", "host tables");
    }
    if (err)
    {
        lthip_restore_destroy(r); // (waits for what was queued; nothing stays allocated)
        return err;
    }
    *out = r;
    return 0;
}

extern "C" int lthip_restore_create(lthip_ctx* ctx, const lthip_restore_config* cfg, const void* version_index, size_t vi_size,
                                    const void* store_index, size_t si_size, const uint64_t* asset_offsets, uint64_t out_bytes, lthip_restore** out)
{
    return restore_create(ctx, cfg, nullptr, version_index, vi_size, store_index, si_size,
                          Wanted{"lthip_restore_create", asset_offsets, false, 0, nullptr}, out_bytes, out);
}

static_assert(sizeof(lthip_restore_window) == sizeof(restore_windows::Window) &&
                  offsetof(lthip_restore_window, dst) == offsetof(restore_windows::Window, dst),
              "restore_windows.h restates lthip_restore_window");

extern "C" int lthip_restore_create_windows(lthip_ctx* ctx, const lthip_restore_config* cfg, const void* version_index, size_t vi_size,
                                            const void* store_index, size_t si_size, uint64_t window_count, const lthip_restore_window* windows,
                                            uint64_t out_bytes, lthip_restore** out)
{
    return restore_create(ctx, cfg, nullptr, version_index, vi_size, store_index, si_size,
                          Wanted{"lthip_restore_create_windows", nullptr, true, window_count,
                                 reinterpret_cast<const restore_windows::Window*>(windows)},
                          out_bytes, out);
}

extern "C" int lthip_restore_asset_sizes(const void* version_index, size_t size, uint64_t* sizes, uint32_t* asset_count, uint32_t* target_chunk_size)
{
    return restore_windows::asset_sizes(version_index, size, sizes, asset_count, target_chunk_size);
}

extern "C" int lthip_restore_rank_windows(uint64_t job_count, const uint32_t* job_asset, const uint64_t* job_offset, const uint64_t* job_size,
                                          const uint32_t* job_rank, uint32_t rank, uint64_t align, lthip_restore_window* windows, uint64_t capacity,
                                          uint64_t* window_count, uint64_t* out_bytes)
{
    return restore_windows::rank_windows(job_count, job_asset, job_offset, job_size, job_rank, rank, align,
                                         reinterpret_cast<restore_windows::Window*>(windows), capacity, window_count, out_bytes);
}

extern "C" int lthip_restore_create_from_base(lthip_ctx* ctx, const lthip_restore_config* cfg, const lthip_restore_base* base,
                                              const void* version_index, size_t vi_size, const void* store_index, size_t si_size,
                                              const uint64_t* asset_offsets, uint64_t out_bytes, lthip_restore** out)
{
    if (out)
        *out = nullptr;
    if (!base || !base->version_index)
        return EINVAL;
    return restore_create(ctx, cfg, base, version_index, vi_size, store_index, si_size,
                          Wanted{"lthip_restore_create_from_base", asset_offsets, false, 0, nullptr}, out_bytes, out);
}

extern "C" int lthip_restore_needed_blocks(const lthip_restore* r, uint64_t* block_hashes, uint64_t capacity, uint64_t* out_count)
{
    if (!r || !out_count)
        return EINVAL;
    *out_count = r->needed;
    if (!block_hashes || capacity < r->needed)
        return 0;
    uint64_t k = 0;
    for (uint32_t b = 0; b < r->nb; ++b)
        if (r->is_needed(b))
            block_hashes[k++] = r->bhash[b];
    return 0;
}

extern "C" size_t lthip_restore_scratch_bound(const lthip_restore* r, uint32_t block_count, const uint64_t* block_hashes)
{
    if (!r || (block_count && !block_hashes))
        return 0;
    uint64_t bytes = 0;
    for (uint32_t i = 0; i < block_count; ++i)
    {
        const auto it = r->block_of_hash.find(block_hashes[i]);
        if (it != r->block_of_hash.end() && r->is_needed(it->second) && r->btag[it->second] != 0u)
            bytes += round64(r->braw[it->second]);
    }
    return (size_t)bytes;
}

static int restore_queue(lthip_restore* r, uint32_t block_count, const uint64_t* block_hashes, const void* d_images, const uint64_t* image_offsets,
                         const uint32_t* image_sizes, void* d_scratch, void* d_out)
{
    lthip_ctx* ctx = r->ctx;
    // ---- the call's needed blocks in three groups: not decoded (raw blocks; an image too short to hold a payload), LZ4, zstd ----
    for (auto& g : r->group)
        g.clear();
    for (uint32_t i = 0; i < block_count; ++i)
    {
        const uint32_t b = r->block_of_hash.find(block_hashes[i])->second;
        r->delivered[b] = 1;
        ++r->delivered_all;
        if (!r->is_needed(b))
        {
            ++r->unneeded;
            continue;
        }
        ++r->needed_delivered;
        const int codec = codec_of_tag(r->btag[b]);
        const bool payload = (uint64_t)image_sizes[i] > lthip_stored_block_header_size(r->bcnt[b]);
        r->group[codec == LTHIP_CODEC_NONE || !payload ? 0 : codec == LTHIP_CODEC_LZ4 ? 1 : 2].push_back(i);
    }
    r->finished = false;
    const size_t k = r->group[0].size() + r->group[1].size() + r->group[2].size();
    if (!k)
        return 0;
    r->blocks_queued = true;
    r->items.clear(), r->outsz.clear();
    uint64_t slot = 0, entries = 0, ranges = 0, leaves = 0;
    for (int g = 0; g < 3; ++g)
        for (const uint32_t i : r->group[g])
        {
            const uint32_t b = r->block_of_hash.find(block_hashes[i])->second;
            const bool tagged = r->btag[b] != 0u;
            RItem it;
            it.image = image_offsets[i];
            it.src = tagged ? (uint64_t)(uintptr_t)d_scratch + slot : (uint64_t)(uintptr_t)d_images + image_offsets[i] + lthip_block_index_size(r->bcnt[b]);
            it.size = image_sizes[i];
            it.block = b;
            it.raw = r->braw[b];
            it.efirst = (uint32_t)entries;
            it.ebase = r->firsts[b];
            it.vfirst = (uint32_t)ranges;
            r->items.push_back(it);
            r->outsz.push_back(tagged ? NONE : it.raw); // (a decoder overwrites its blocks' words; a raw block has nothing to decode)
            if (tagged)
                slot += round64(it.raw);
            entries += r->firsts[b + 1] - r->firsts[b];
            ranges += r->bcnt[b];
            leaves += r->bleaves[b];
        }
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int err;
    if ((err = upload(ctx, r->d_items, r->items.data(), k * sizeof(RItem))) || (err = upload(ctx, r->d_outsz, r->outsz.data(), k * 4)))
        return err;
    {
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_restore_check_images, dim3((uint32_t)k), dim3(64), 0, s, (const RItem*)r->d_items, (uint32_t)k, (const uint8_t*)d_images,
                           (const uint64_t*)r->d_bhash, (const uint32_t*)r->d_bcoff, (const uint32_t*)r->d_bcnt, (const uint32_t*)r->d_btag,
                           (const uint32_t*)r->d_braw, r->hash_identifier, (const uint64_t*)r->d_chash, (const uint32_t*)r->d_csize, r->d_status);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    // ---- decode: one call per codec; sizes and places from the StoreIndex and image_sizes alone ----
    size_t at = r->group[0].size();
    for (int g = 1; g < 3; ++g)
    {
        const size_t cnt = r->group[g].size();
        if (!cnt)
            continue;
        r->c_src.clear(), r->c_size.clear(), r->c_dst.clear(), r->c_cap.clear();
        for (size_t j = 0; j < cnt; ++j)
        {
            const RItem& it = r->items[at + j];
            const uint64_t hdr = lthip_stored_block_header_size(r->bcnt[it.block]);
            r->c_src.push_back(it.image + hdr);
            r->c_size.push_back((uint32_t)(it.size - hdr));
            r->c_dst.push_back(it.src - (uint64_t)(uintptr_t)d_scratch);
            r->c_cap.push_back(it.raw);
        }
        err = g == 1 ? lthip_lz4_decompress_blocks(ctx, d_images, (uint32_t)cnt, r->c_src.data(), r->c_size.data(), d_scratch, r->c_dst.data(),
                                                   r->c_cap.data(), r->d_outsz + at)
                     : lthip_zstd_decompress_blocks(ctx, d_images, (uint32_t)cnt, r->c_src.data(), r->c_size.data(), d_scratch, r->c_dst.data(),
                                                    r->c_cap.data(), r->d_outsz + at);
        if (err)
            return err;
        at += cnt;
    }
    // ---- the decoders' verdict, then verify, both before the scatter ----
    const uint64_t base = slot ? std::min((uint64_t)(uintptr_t)d_images, (uint64_t)(uintptr_t)d_scratch) : (uint64_t)(uintptr_t)d_images;
    {
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_restore_ranges, dim3((uint32_t)k), dim3(64), 0, s, (const RItem*)r->d_items, (uint32_t)k, (const uint32_t*)r->d_outsz,
                           (const uint32_t*)r->d_bcoff, (const uint32_t*)r->d_bcnt, (const uint32_t*)r->d_csize, (const uint32_t*)r->d_coff, r->d_status,
                           r->verify, base, r->d_voff, r->d_vlen, r->d_vblock, r->d_vchunk);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if (r->verify && ranges)
    {
        if ((err = lthip_hash_ranges_by_id(ctx, r->hash_identifier, (const void*)(uintptr_t)base, ranges, r->d_voff, r->d_vlen, r->max_chunk, leaves,
                                           r->d_vhash)))
            return err;
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_restore_compare, dim3((uint32_t)((ranges + 255u) / 256u)), dim3(256), 0, s, (uint32_t)ranges, (const uint64_t*)r->d_vhash,
                           (const uint32_t*)r->d_vblock, (const uint32_t*)r->d_vchunk, (const uint64_t*)r->d_chash, r->d_status, r->d_counters + 1);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    LaunchTimer tm(ctx, LTHIP_K_GATHER);
    constexpr uint64_t LAUNCH_ENTRIES = 1u << 23; // (a launch holds fewer than 2^32 threads)
    for (uint64_t e0 = 0; e0 < entries; e0 += LAUNCH_ENTRIES)
        hipLaunchKernelGGL(k_restore_scatter, dim3((uint32_t)std::min(LAUNCH_ENTRIES, entries - e0)), dim3(RT), 0, s, (const RItem*)r->d_items,
                           (uint32_t)k, (const uint4*)r->d_entries, (const uint32_t*)r->d_status, (const uint32_t*)r->d_outsz, (uint32_t)e0,
                           (uint8_t*)d_out);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

extern "C" int lthip_restore_blocks(lthip_restore* r, uint32_t block_count, const uint64_t* block_hashes, const void* d_images,
                                    const uint64_t* image_offsets, const uint32_t* image_sizes, void* d_scratch, uint64_t scratch_bytes, void* d_out)
{
    if (!r || (block_count && (!block_hashes || !d_images || !image_offsets || !image_sizes)))
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    // ---- the refusals, before anything is queued or changed ----
    int refused = 0;
    const char* why = "";
    uint64_t scratch = 0;
    bool any_needed = false;
    uint32_t marked = 0;
    for (; marked < block_count && !refused; ++marked)
    {
        const auto it = r->block_of_hash.find(block_hashes[marked]);
        if (it == r->block_of_hash.end())
        {
            refused = ENOENT, why = "a block hash the store index does not hold";
            break;
        }
        const uint32_t b = it->second;
        if (r->delivered[b] || r->in_call[b])
        {
            refused = EEXIST, why = "a block was delivered before, or twice in this call";
            break;
        }
        r->in_call[b] = 1;
        if (image_offsets[marked] & 7u)
            refused = EINVAL, why = "image offsets must be 8-byte aligned";
        else if (r->is_needed(b))
        {
            any_needed = true;
            if (codec_of_tag(r->btag[b]) < 0)
                refused = ENOTSUP, why = "a needed block's tag names no codec of this library";
            else if (r->btag[b] != 0u)
                scratch += round64(r->braw[b]);
        }
    }
    for (uint32_t i = 0; i < block_count && i <= marked; ++i) // (the marks of this call, the refused block's included)
    {
        const auto it = r->block_of_hash.find(block_hashes[i]);
        if (it != r->block_of_hash.end() && !r->delivered[it->second])
            r->in_call[it->second] = 0;
    }
    if (!refused && scratch > scratch_bytes)
        refused = ENOMEM, why = "scratch below lthip_restore_scratch_bound";
    if (!refused && ((scratch && !d_scratch) || (any_needed && !d_out)))
        refused = EINVAL, why = "null scratch or output";
    if (!refused && any_needed && r->in_place_buf && d_out != r->in_place_buf)
        refused = EINVAL, why = "the base was carried in place: the output is that buffer";
    if (refused)
        return lthip_fail(ctx, refused, "lthip_restore_blocks", why);
    try
    {
        return restore_queue(r, block_count, block_hashes, d_images, image_offsets, image_sizes, d_scratch, d_out);
    }
    catch (const std::bad_alloc&)
    {
        return lthip_fail(ctx, ENOMEM, "lthip_restore_blocks", "host tables");
    }
}

// d_scratch == null: out of place, d_base -> d_out.  Otherwise in place: d_base == d_out is the one buffer, and the moved runs go through
// d_scratch (16-byte aligned, lthip_restore_in_place_scratch_bound), all reads before all writes.
static int carry_queue(lthip_restore* r, const void* d_base, void* d_out, void* d_scratch)
{
    lthip_ctx* ctx = r->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const uint32_t n = r->ncarry;
    const size_t n2 = ((size_t)n + 2) & ~(size_t)1;
    const bool in_place = r->in_place;
    int err;
    // ---- verify: the base chunks that feed something, hashed where they lie, before anything of them is copied ----
    const uint32_t* bbad = nullptr;
    if (r->verify && r->nmarked)
    {
        if ((err = lthip_hash_ranges_by_id(ctx, r->hash_identifier, d_base, r->nmarked, r->d_cvoff, r->d_cvlen, r->base_max_chunk, r->carry_leaves,
                                           r->d_cvhash)))
            return err;
        LaunchTimer tm(ctx, LTHIP_K_OTHER);
        hipLaunchKernelGGL(k_restore_carry_compare, dim3((r->nmarked + 255u) / 256u), dim3(256), 0, s, r->nmarked, (const uint64_t*)r->d_cvhash,
                           (const uint32_t*)r->d_cvchunk, (const uint64_t*)r->d_uhash, (const uint32_t*)r->d_usize, (const uint32_t*)r->d_ufeed,
                           r->d_ubad, r->d_counters);
        LTHIP_LAUNCH_CHECK(ctx);
        bbad = r->d_ubad;
    }
    if (in_place && !r->moved_occ) // everything the base feeds lies where it belongs: no copy is queued
        return 0;
    // [n u64 run source][n u64 run destination][n u64 run length][n u32 pieces][n + 1 u32 first piece][n u32 boundary][n + 1 u32 rank]
    // in place, behind them: [n u64 run slot][n u32 pieces in][n + 1 u32 first piece in][n u32 units][n + 1 u32 first unit]
    void* tab = nullptr;
    if ((err = lthip_scratch(ctx, S_CARRY_RUNS, n2 * (in_place ? 64 : 40), &tab)))
        return err;
    uint64_t* run_src = (uint64_t*)tab;
    uint64_t* run_dst = run_src + n2;
    uint64_t* run_len = run_dst + n2;
    uint32_t* pieces = (uint32_t*)(run_len + n2);
    uint32_t* first_piece = pieces + n2;
    uint32_t* bound = first_piece + n2;
    uint32_t* rank = bound + n2;
    // ---- runs: boundaries, their scan, a slot per entry that starts a run, the pieces' scan, the copy ----
    {
        LaunchTimer tm(ctx, LTHIP_K_GATHER);
        hipLaunchKernelGGL(k_restore_carry_bounds, dim3((n + 255u) / 256u), dim3(256), 0, s, n, (const uint64_t*)r->d_ksrc, (const uint64_t*)r->d_kdst,
                           (const uint32_t*)r->d_klen, (const uint32_t*)r->d_kchunk, bbad, bound);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if ((err = lthip_exclusive_scan_u32(ctx, bound, rank, n, nullptr, LTHIP_K_GATHER)))
        return err;
    {
        LaunchTimer tm(ctx, LTHIP_K_GATHER);
        hipLaunchKernelGGL(k_restore_carry_runs, dim3((n + 255u) / 256u), dim3(256), 0, s, n, (const uint64_t*)r->d_ksrc, (const uint64_t*)r->d_kdst,
                           (const uint32_t*)r->d_klen, (const uint32_t*)r->d_kchunk, bbad, (const uint32_t*)bound, (const uint32_t*)rank, run_src,
                           run_dst, run_len, pieces);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if (!in_place)
    {
        if ((err = lthip_exclusive_scan_u32(ctx, pieces, first_piece, n, nullptr, LTHIP_K_GATHER)))
            return err;
        return lthip_raw_copy_runs(ctx, first_piece, n, run_src, run_dst, run_len, d_base, d_out, r->carry_bytes / (LTHIP_RAW_PIECE_VEC * 16u) + n);
    }
    // ---- in place: kept runs drop out, moved runs get a slot; pass 1 buffer -> scratch, pass 2 scratch -> buffer ----
    uint64_t* run_slot = (uint64_t*)(rank + n2);
    uint32_t* pieces_in = (uint32_t*)(run_slot + n2);
    uint32_t* first_piece_in = pieces_in + n2;
    uint32_t* units = first_piece_in + n2;
    uint32_t* first_unit = units + n2;
    {
        LaunchTimer tm(ctx, LTHIP_K_GATHER);
        hipLaunchKernelGGL(k_restore_in_place_classify, dim3((n + 255u) / 256u), dim3(256), 0, s, n, (const uint64_t*)run_src,
                           (const uint64_t*)run_dst, (const uint64_t*)run_len, pieces, pieces_in, units);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    if ((err = lthip_exclusive_scan_u32(ctx, units, first_unit, n, nullptr, LTHIP_K_GATHER)) ||
        (err = lthip_exclusive_scan_u32(ctx, pieces_in, first_piece_in, n, nullptr, LTHIP_K_GATHER)) ||
        (err = lthip_exclusive_scan_u32(ctx, pieces, first_piece, n, nullptr, LTHIP_K_GATHER)))
        return err;
    {
        LaunchTimer tm(ctx, LTHIP_K_GATHER);
        hipLaunchKernelGGL(k_restore_in_place_slots, dim3((n + 255u) / 256u), dim3(256), 0, s, n, (const uint32_t*)first_unit, run_slot);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    const uint64_t pieces_bound = r->moved_bytes / (LTHIP_RAW_PIECE_VEC * 16u) + r->moved_occ;
    if ((err = lthip_raw_copy_runs(ctx, first_piece_in, n, run_src, run_slot, run_len, d_base, d_scratch, pieces_bound)))
        return err;
    return lthip_raw_copy_runs(ctx, first_piece, n, run_slot, run_dst, run_len, d_scratch, d_out, pieces_bound);
}

extern "C" int lthip_restore_carry(lthip_restore* r, const void* d_base, void* d_out)
{
    if (!r)
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    // ---- the refusals, before anything is queued or changed ----
    if (!r->has_base)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry", "the session was created without a base");
    if (r->carried)
        return lthip_fail(ctx, EEXIST, "lthip_restore_carry", "the base was carried before");
    if (r->ncarry)
    {
        if (!d_base || !d_out)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry", "null base or output");
        const uint64_t b0 = (uint64_t)(uintptr_t)d_base, o0 = (uint64_t)(uintptr_t)d_out;
        if (b0 < o0 + r->out_bytes && o0 < b0 + r->base_window)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry", "the base and the output overlap: the update is out of place");
        const int err = carry_queue(r, d_base, d_out, nullptr);
        if (err)
            return err;
    }
    r->carried = true;
    r->finished = false;
    return 0;
}

// what the moved runs need in the caller's scratch: their bytes, every run's slot rounded up to 16 bytes (a run holds at least one moved
// occurrence), and room to start the first slot on a 16-byte boundary
static uint64_t in_place_bound(const lthip_restore* r) { return r->moved_occ ? r->moved_bytes + 16u * r->moved_occ + 64u : 0u; }

extern "C" size_t lthip_restore_in_place_scratch_bound(const lthip_restore* r) { return r && r->has_base ? (size_t)in_place_bound(r) : 0; }

extern "C" int lthip_restore_in_place_stats(const lthip_restore* r, uint64_t out[4])
{
    if (!r || !out)
        return EINVAL;
    out[0] = r->has_base ? r->ncarry - r->moved_occ : 0u;
    out[1] = r->has_base ? r->carry_bytes - r->moved_bytes : 0u;
    out[2] = r->has_base ? r->moved_occ : 0u;
    out[3] = r->has_base ? r->moved_bytes : 0u;
    return 0;
}

extern "C" int lthip_restore_carry_in_place(lthip_restore* r, void* d_buf, void* d_scratch, uint64_t scratch_bytes)
{
    if (!r)
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    // ---- the refusals, before anything is queued or changed ----
    if (!r->has_base)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "the session was created without a base");
    if (r->carried)
        return lthip_fail(ctx, EEXIST, "lthip_restore_carry_in_place", "the base was carried before");
    if (r->blocks_queued)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "a blocks call has queued work: the carry in place comes first");
    if (r->ncarry && !d_buf)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "null buffer");
    void* scratch = nullptr;
    if (r->moved_occ)
    {
        const uint64_t bound = in_place_bound(r);
        if (bound >> 36) // (the slots are placed by a 32-bit scan of 16-byte units)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "more than 64 GiB would move: update out of place");
        if (!d_scratch)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "null scratch");
        const uint64_t b0 = (uint64_t)(uintptr_t)d_buf, s0 = (uint64_t)(uintptr_t)d_scratch;
        if (s0 < b0 + std::max(r->base_window, r->out_bytes) && b0 < s0 + std::max(bound, scratch_bytes))
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "the scratch overlaps the buffer");
        if (scratch_bytes < bound)
            return lthip_fail(ctx, ENOMEM, "lthip_restore_carry_in_place", "scratch below lthip_restore_in_place_scratch_bound");
        scratch = (void*)(uintptr_t)((s0 + 15u) & ~(uint64_t)15u);
    }
    r->in_place = true;
    const int err = r->ncarry ? carry_queue(r, d_buf, d_buf, scratch) : 0;
    if (err)
    {
        r->in_place = false;
        return err;
    }
    r->in_place_buf = d_buf;
    r->carried = true;
    r->finished = false;
    return 0;
}

extern "C" int lthip_restore_layout_in_place(const void* base_vi, size_t base_vi_size, const uint64_t* base_offsets, uint64_t base_bytes,
                                             const void* target_vi, size_t target_vi_size, uint64_t align, uint64_t* target_offsets,
                                             uint32_t* asset_count, uint64_t* total_bytes, uint32_t* kept_assets)
{
    try
    {
        return restore_layout::in_place(base_vi, base_vi_size, base_offsets, base_bytes, target_vi, target_vi_size, align, target_offsets, asset_count,
                                        total_bytes, kept_assets);
    }
    catch (const std::bad_alloc&)
    {
        return ENOMEM;
    }
}

extern "C" int lthip_version_diff(const void* source_vi, size_t source_size, const void* target_vi, size_t target_size, uint32_t* source_removed,
                                  uint32_t* target_added, uint32_t* source_content_modified, uint32_t* target_content_modified,
                                  uint32_t* source_permissions_modified, uint32_t* target_permissions_modified, uint32_t counts[4])
{
    if (!source_vi || !target_vi || !counts)
        return EINVAL;
    try
    {
        version_diff::Lists d;
        const int err = version_diff::diff(source_vi, source_size, target_vi, target_size, &d);
        if (err)
            return err;
        const std::vector<uint32_t>* lists[6] = {&d.source_removed, &d.target_added, &d.source_content, &d.target_content, &d.source_permissions,
                                                 &d.target_permissions};
        uint32_t* outs[6] = {source_removed, target_added, source_content_modified, target_content_modified, source_permissions_modified,
                             target_permissions_modified};
        for (int k = 0; k < 6; ++k)
            if (outs[k] && !lists[k]->empty())
                memcpy(outs[k], lists[k]->data(), lists[k]->size() * 4);
        counts[0] = (uint32_t)d.source_removed.size(), counts[1] = (uint32_t)d.target_added.size();
        counts[2] = (uint32_t)d.source_content.size(), counts[3] = (uint32_t)d.source_permissions.size();
        return 0;
    }
    catch (const std::bad_alloc&)
    {
        return ENOMEM;
    }
}

extern "C" int lthip_restore_finish(lthip_restore* r, lthip_restore_result* out)
{
    if (!r || (out && (out->struct_size < 16 || out->struct_size > 4096)))
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    unsigned long long counters[5] = {0}; // (d_counters' [1] .. [4])
    if (r->nb)
        LTHIP_CHECK(ctx, hipMemcpyAsync(r->status.data(), r->d_status, (size_t)r->nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    LTHIP_CHECK(ctx, hipMemcpyAsync(counters + 1, r->d_counters + 1, 32, hipMemcpyDeviceToHost, ctx->stream));
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    r->finished = true;
    lthip_restore_result res;
    memset(&res, 0, sizeof res);
    res.assets_selected = r->assets_selected;
    res.occurrences = r->nocc;
    res.blocks_needed = r->needed;
    res.blocks_delivered = r->delivered_all;
    res.blocks_unneeded = r->unneeded;
    res.chunks_mismatched = counters[1];
    res.base_occurrences = r->ncarry;
    res.base_bytes = r->carry_bytes;
    res.base_chunks_mismatched = counters[2];
    if (r->carried) // (what a mismatched base chunk would have fed was left out of the runs)
    {
        res.occurrences_written = r->ncarry - counters[3];
        res.bytes_written = r->carry_bytes - counters[4];
    }
    for (uint32_t b = 0; b < r->nb; ++b)
    {
        if (!r->delivered[b] || !r->is_needed(b))
            continue;
        if (r->status[b])
            ++res.blocks_bad;
        else
        {
            res.occurrences_written += r->firsts[b + 1] - r->firsts[b];
            res.bytes_written += r->bbytes[b];
        }
        if (r->btag[b] != 0u && !(r->status[b] & (LTHIP_RESTORE_BAD_HEADER | LTHIP_RESTORE_BAD_PAYLOAD)))
            res.decoded_bytes += r->braw[b];
    }
    if (out)
    {
        const uint64_t have = out->struct_size;
        res.struct_size = have < sizeof res ? have : sizeof res;
        memcpy(out, &res, (size_t)res.struct_size);
    }
    return res.blocks_bad || res.base_chunks_mismatched ? EBADF : r->needed_delivered < r->needed || (r->ncarry && !r->carried) ? ENOENT : 0;
}

extern "C" int lthip_restore_block_status(const lthip_restore* r, uint32_t count, const uint64_t* block_hashes, uint32_t* status)
{
    if (!r || (count && (!block_hashes || !status)))
        return EINVAL;
    if (!r->finished)
        return lthip_fail(r->ctx, EINVAL, "lthip_restore_block_status", "valid after lthip_restore_finish");
    for (uint32_t i = 0; i < count; ++i)
    {
        const auto it = r->block_of_hash.find(block_hashes[i]);
        if (it == r->block_of_hash.end())
            return lthip_fail(r->ctx, ENOENT, "lthip_restore_block_status", "a block hash the store index does not hold");
        const uint32_t b = it->second;
        status[i] = !r->is_needed(b) ? 0u : !r->delivered[b] ? LTHIP_RESTORE_NOT_DELIVERED : r->status[b];
    }
    return 0;
}
