// restore.hip -- the restore session (include/longtail_hip.h, "the restore session"): stored-block images in HBM back into the assets of
// a version, the device side of Longtail_WriteVersion (src/longtail.c:6471-6573; BuildAssetWriteList :6021, WriteAssetsFromBlock :5700)
// and DecompressBlock (compressblockstore.c:271-338).
//
//   create   the host expands the VersionIndex into OCCURRENCES (chunk hash, destination, length) -- prefix arithmetic over
//            m_AssetChunkIndexes and m_ChunkSizes, restore_windows.h -- and the StoreIndex into per-chunk (block, offset in block),
//            restore_plan.h: the plan's host tables are plain headers that a sanitizer reaches without a GPU.  The device resolves: the
//            StoreIndex's chunk hashes go into an lthip_seen, lthip_seen_find gives every occurrence the position of its chunk,
//            k_restore_resolve checks the size and counts occurrences per block, an exclusive scan gives every block its first entry,
//            k_restore_fill places (offset in block, length, destination) block-major; where an occurrence comes from is decided by one
//            routine, resolve(), for both.  The block_count + 1 firsts come back once.
//   windows  (lthip_restore_create_windows, restore_windows.h) the occurrences are those of byte windows of assets, each CLIPPED to its
//            window: next to the chunk's full length it carries `skip` bytes into the chunk and `clip` bytes to write.  k_restore_resolve
//            still compares the full length with the StoreIndex's size and counts `clip` bytes; k_restore_fill places (offset in block +
//            skip, clip, destination).  A clipped occurrence is an ordinary entry: check, decode, verify and scatter do not know of it.
//            The sessions of whole assets are the same routine with one window per selected asset and no skip / clip tables at all.
//   list     (lthip_restore_create_occurrences, lthip_internal.h) the occurrences lie on the device already -- the repack session's moved
//            chunks, each a whole chunk with a destination in its work buffer: no VersionIndex is read and nothing is expanded, the
//            list is copied device to device into the plan's tables and everything behind that is the same plan.
//   blocks   k_restore_check_images (a wave per image, against the device copy of the StoreIndex) -> the decoders into 64-byte slots of
//            the caller's scratch -> k_restore_ranges (the decoders' verdict into the block's status word; with verify the (offset,
//            length) of every chunk) -> lthip_hash_ranges_by_id -> k_restore_compare -> k_restore_scatter over the call's entries
//            (the copy: lthip_wg_copy, k_copy.h).  Nothing is allocated and nothing is waited for: the session's tables were sized by
//            create.
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
// Device tables travel to the kernels as views by value, what the kernels count for the host has names (Counters), and every table set
// is sub-allocated by a Carver: the session's allocation, the plan's temporaries, the carry's tables in the context's scratch.
// The scatter and a decoder's second pass cost one more read and write of the output than decoding into place would: about a tenth on top
// of the bare decoder calls (profiles/restore_rate.json).
//   cache    (lthip_block_cache, lthip_restore_set_cache; the bookkeeping is host code, block_cache.h) a device arena of slots of one
//            size that outlives the sessions.  A slot is a third kind of RItem::src.  set_cache looks every needed block up: a matching
//            entry is pinned, the block is CACHE-FED and no longer needed; lthip_restore_from_cache scatters those from their slots with
//            k_restore_scatter over an item table of its own.  A blocks call reserves a slot per needed block: a tagged block is decoded
//            into it (the decoders' one destination base becomes the lower of scratch and arena), a raw block's payload is copied into
//            it by k_restore_cache_copy behind the check.  finish, which reads the status words anyway, commits the good ones.
//            Without a cache attached restore_queue computes what it always did.
//   archive  (lthip_restore_archive_blocks; the index is host code, archive_layout.h) the images lie in the body of a one-file archive,
//            back to back at ANY byte position.  The host picks the needed, undelivered blocks that lie wholly inside the caller's window
//            of the body and delivers them through the routine lthip_restore_blocks uses, without its alignment refusal; the one stage
//            that cared, the check, runs as k_restore_check_images_any: every header dword from the two aligned dwords around it.
//   call     (restore_call.h, host code) what a blocks call names, whether it is refused and what it changes: lthip_restore_blocks
//            resolves its hashes to block indices once, the archive's pick yields indices; restore_deliver and restore_queue take those.
//            restore_queue is five stages -- items and slots, check, decode, judge, scatter -- of which only the last knows of entries.
#include "archive_layout.h"
#include "block_cache.h"
#include "k_copy.h"
#include "lthip_internal.h"
#include "restore_call.h"
#include "restore_layout.h"
#include "version_diff.h"

namespace
{

using restore_plan::NONE;
using restore_plan::NOWHERE;
constexpr int RT = 256;

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

// what the kernels count for the host: the plan's one read-back takes all of it, lthip_restore_finish the mismatches
struct Counters
{
    unsigned long long unresolved;         // occurrences neither source resolves
    unsigned long long block_chunks_bad;   // chunks of blocks whose hash differed
    unsigned long long base_chunks_bad;    // base chunks whose hash differed,
    unsigned long long base_bad_occ;       // the occurrences those would have fed
    unsigned long long base_bad_bytes;     // and their bytes
    unsigned long long base_bytes;         // bytes the base feeds
    unsigned long long base_verify_leaves; // 1 KiB leaves of the base chunks that feed (lthip_hash_ranges_by_id wants the total)
    unsigned long long moved_occ;          // base-fed entries whose source offset is not their destination (an update in place copies
    unsigned long long moved_bytes;        // them) and their bytes
};

// sub-allocation of one device allocation.  A table set's carve(Carver(), ...) takes nothing and returns the bytes it needs;
// carve(Carver(memory), ...) makes the same calls again and hands out the pieces.
struct Carver
{
    uint8_t* p;
    size_t at = 0;
    explicit Carver(void* memory = nullptr) : p((uint8_t*)memory) {}
    template <class T> void take(T** out, size_t count)
    {
        if (p)
            *out = reinterpret_cast<T*>(p + at);
        at += (count * sizeof(T) + 255u) & ~(size_t)255u;
    }
};

// ---- device tables, handed to the kernels by value ----
// the StoreIndex: per chunk position (hash, size, the block that holds it or NONE, offset in that block), per block (hash, first chunk
// position, chunk count, tag, raw size)
struct StoreView
{
    uint64_t *chash = nullptr, *bhash = nullptr;
    uint32_t *csize = nullptr, *cblock = nullptr, *coff = nullptr, *bcoff = nullptr, *bcnt = nullptr, *btag = nullptr, *braw = nullptr;
};
// the occurrences: position of the chunk in the StoreIndex's chunk list (lthip_seen_find) and among the base's chunks (null without a
// base), the chunk's FULL length, destination; skip / clip: what a clipped occurrence leaves out and writes, null when every occurrence
// is its whole chunk
struct OccView
{
    uint32_t *pos = nullptr, *bpos = nullptr, *len = nullptr, *skip = nullptr, *clip = nullptr;
    uint64_t* dst = nullptr;
};
// per distinct chunk of the base {hash, size, offset of its first resident occurrence (NOWHERE: none), occurrences fed, hash differed}
struct BaseView
{
    uint64_t *hash = nullptr, *off = nullptr;
    uint32_t *size = nullptr, *feed = nullptr, *bad = nullptr;
};
// base-fed entries in occurrence order (room for every occurrence: how many the base feeds is known after the plan has run)
struct CarryView
{
    uint64_t *src = nullptr, *dst = nullptr;
    uint32_t *len = nullptr, *chunk = nullptr;
};
// the byte ranges verify hashes: the chunks of a call's blocks, or (block unused) the base chunks that feed something
struct RangeView
{
    uint64_t *off = nullptr, *hash = nullptr;
    uint32_t *len = nullptr, *block = nullptr, *chunk = nullptr;
};

// ---- plan ----
// what only the plan needs, in an allocation of its own
struct PlanTmp
{
    uint64_t* ohash = nullptr;
    OccView occ;
    unsigned long long* bbytes = nullptr;                   // per block: the bytes its entries write
    uint32_t *hist = nullptr, *cursor = nullptr;            // per block: its entries counted, and handed out
    uint32_t *first = nullptr, *bfirst = nullptr;           // lthip_seen_add's answers, not read
    uint32_t *oflag = nullptr, *ofirst = nullptr;           // per occurrence: the base feeds it, and the scan of that
    uint32_t *bmark = nullptr, *mfirst = nullptr;           // per base chunk: it feeds something, and the scan of that
    size_t carve(Carver c, size_t nocc, size_t nb, size_t m, size_t nub, bool clipped, bool base)
    {
        c.take(&ohash, nocc), c.take(&occ.dst, nocc), c.take(&bbytes, nb), c.take(&occ.len, nocc), c.take(&occ.pos, nocc), c.take(&hist, nb),
            c.take(&cursor, nb), c.take(&first, m);
        if (clipped)
            c.take(&occ.skip, nocc), c.take(&occ.clip, nocc);
        if (base)
            c.take(&occ.bpos, nocc), c.take(&oflag, nocc), c.take(&ofirst, nocc + 1), c.take(&bfirst, nub), c.take(&bmark, nub),
                c.take(&mfirst, nub + 1);
        return c.at;
    }
};

// where occurrence i comes from.  q != NONE: base chunk q -- the base holds its hash with the same size at a resident offset, and wins
// when both hold the chunk.  Else b != NONE: position p of the StoreIndex's chunk list, in block b.  Else nowhere.
struct Resolved
{
    uint32_t q, p, b;
};
__device__ __forceinline__ Resolved resolve(const OccView& o, const BaseView& base, const StoreView& sv, uint32_t i)
{
    const uint32_t len = o.len[i], q = o.bpos ? o.bpos[i] : NONE;
    if (q != NONE && base.size[q] == len && base.off[q] != NOWHERE)
        return Resolved{q, NONE, NONE};
    const uint32_t p = o.pos[i];
    const uint32_t b = p == NONE ? NONE : sv.cblock[p];
    return b != NONE && sv.csize[p] == len ? Resolved{NONE, p, b} : Resolved{NONE, NONE, NONE};
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int o = 32; o; o >>= 1)
        v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void k_restore_resolve(uint32_t n, PlanTmp t, BaseView base, StoreView sv, Counters* counters)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    unsigned long long fed = 0;
    if (i < n)
    {
        const uint32_t len = t.occ.len[i];
        const Resolved r = resolve(t.occ, base, sv, i);
        if (t.oflag)
            t.oflag[i] = r.q != NONE ? 1u : 0u;
        if (r.q != NONE)
        {
            atomicAdd(&base.feed[r.q], 1u);
            t.bmark[r.q] = 1u;
            fed = len;
        }
        else if (r.b == NONE)
            miss = true;
        else
        {
            atomicAdd(&t.hist[r.b], 1u);
            atomicAdd(&t.bbytes[r.b], (unsigned long long)(t.occ.clip ? t.occ.clip[i] : len));
        }
    }
    const uint64_t m = __builtin_amdgcn_ballot_w64(miss);
    if (m && (threadIdx.x & 63) == 0)
        atomicAdd(&counters->unresolved, (unsigned long long)__builtin_popcountll(m));
    if (t.occ.bpos)
    {
        fed = wave_sum(fed);
        if (fed && (threadIdx.x & 63) == 0)
            atomicAdd(&counters->base_bytes, fed);
    }
}

// the order of a block's entries is whatever the atomics give; the output does not depend on it.  The base's entries keep the order of
// the occurrences (ofirst: the scan of the flags): that order is what makes runs.
__global__ void k_restore_fill(uint32_t n, PlanTmp t, BaseView base, StoreView sv, const uint32_t* __restrict__ firsts,
                               uint4* __restrict__ entries, CarryView carry, Counters* counters)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long moved = 0; // bytes of a base-fed entry whose source offset is not its destination
    bool is_moved = false;
    if (i < n)
    {
        const uint32_t len = t.occ.len[i];
        const uint64_t d = t.occ.dst[i];
        const Resolved r = resolve(t.occ, base, sv, i);
        if (r.q != NONE)
        {
            const uint32_t k = t.ofirst[i];
            const uint64_t src = base.off[r.q];
            carry.src[k] = src;
            carry.dst[k] = d;
            carry.len[k] = len;
            carry.chunk[k] = r.q;
            is_moved = src != d;
            moved = is_moved ? len : 0u;
        }
        else if (r.b != NONE)
        {
            const uint32_t slot = firsts[r.b] + atomicAdd(&t.cursor[r.b], 1u);
            // (skip + clip <= len == csize[p]: the entry stays inside its chunk, and the block's raw size is below 2^32)
            const uint32_t skip = t.occ.skip ? t.occ.skip[i] : 0u, clip = t.occ.clip ? t.occ.clip[i] : len;
            entries[slot] = make_uint4(sv.coff[r.p] + skip, clip, (uint32_t)d, (uint32_t)(d >> 32));
        }
    }
    if (!t.occ.bpos)
        return;
    const uint64_t m = __builtin_amdgcn_ballot_w64(is_moved);
    moved = wave_sum(moved);
    if (m && (threadIdx.x & 63) == 0)
    {
        atomicAdd(&counters->moved_occ, (unsigned long long)__builtin_popcountll(m));
        atomicAdd(&counters->moved_bytes, moved);
    }
}

// the base chunks that feed something, in chunk order (mfirst: the scan of their marks): the ranges verify hashes, and their 1 KiB
// leaves summed
__global__ void k_restore_carry_marked(uint32_t n, PlanTmp t, BaseView base, RangeView v, Counters* counters)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long leaves = 0;
    if (q < n && t.bmark[q])
    {
        const uint32_t k = t.mfirst[q], len = base.size[q];
        v.off[k] = base.off[q];
        v.len[k] = len;
        v.chunk[k] = q;
        leaves = len ? ((unsigned long long)len + 1023u) >> 10 : 1u;
    }
    leaves = wave_sum(leaves);
    if (leaves && (threadIdx.x & 63) == 0)
        atomicAdd(&counters->base_verify_leaves, leaves);
}

// ---- carry ----
__global__ void k_restore_carry_compare(uint32_t n, RangeView v, BaseView base, Counters* counters)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n)
        return;
    const uint32_t q = v.chunk[k];
    const bool bad = v.hash[k] != base.hash[q];
    base.bad[q] = bad ? 1u : 0u;
    if (bad)
    {
        atomicAdd(&counters->base_chunks_bad, 1ull);
        atomicAdd(&counters->base_bad_occ, (unsigned long long)base.feed[q]);
        atomicAdd(&counters->base_bad_bytes, (unsigned long long)base.feed[q] * base.size[q]);
    }
}

// the carry's tables in the context's scratch, one slot per base-fed entry: per entry that starts a run {source, destination, length}
// and the run's pieces, the pieces' scan, and what finds the runs: boundary flags and their scan.  In place, behind them: per moved run
// its slot in the caller's scratch, the pieces of its way in and their scan, the 16-byte units of its slot and their scan.
struct RunTables
{
    uint64_t *src = nullptr, *dst = nullptr, *len = nullptr, *slot = nullptr;
    uint32_t *pieces = nullptr, *first_piece = nullptr, *bound = nullptr, *rank = nullptr;
    uint32_t *pieces_in = nullptr, *first_piece_in = nullptr, *units = nullptr, *first_unit = nullptr;
    size_t carve(Carver c, size_t n, bool in_place)
    {
        c.take(&src, n), c.take(&dst, n), c.take(&len, n), c.take(&pieces, n), c.take(&first_piece, n + 1), c.take(&bound, n),
            c.take(&rank, n + 1);
        if (in_place)
            c.take(&slot, n), c.take(&pieces_in, n), c.take(&first_piece_in, n + 1), c.take(&units, n), c.take(&first_unit, n + 1);
        return c.at;
    }
};

// bound[i] = 1: entry i does not continue entry i - 1 -- it starts a run, or (bbad, verify) it is left out and breaks one
__global__ void k_restore_carry_bounds(uint32_t n, CarryView k, const uint32_t* __restrict__ bbad, RunTables runs)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    bool b = i == 0 || (bbad && (bbad[k.chunk[i]] || bbad[k.chunk[i - 1]]));
    if (!b)
    {
        const uint64_t len = k.len[i - 1];
        b = k.src[i] != k.src[i - 1] + len || k.dst[i] != k.dst[i - 1] + len;
    }
    runs.bound[i] = b ? 1u : 0u;
}

// rank = the exclusive scan of bound (n + 1 entries).  A boundary that starts a run ends it before the next boundary: the first j > i
// with rank[j + 1] > rank[i] + 1, found by bisection (rank is monotone), or the end of the list.  The entries of a run follow each other
// in the destination, so its length is the end of its last entry - its start.
__global__ void k_restore_carry_runs(uint32_t n, CarryView k, const uint32_t* __restrict__ bbad, RunTables runs)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t np = 0;
    if (runs.bound[i] && !(bbad && bbad[k.chunk[i]]))
    {
        const uint32_t r = runs.rank[i] + 1u; // boundaries up to and including i
        uint32_t lo = i, hi = n;              // rank[lo + 1] == r (no boundary in (i, lo]); hi == n or rank[hi + 1] > r
        while (hi - lo > 1)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (runs.rank[mid + 1] > r)
                hi = mid;
            else
                lo = mid;
        }
        const uint64_t d = k.dst[i], len = k.dst[lo] + k.len[lo] - d;
        runs.src[i] = k.src[i];
        runs.dst[i] = d;
        runs.len[i] = len;
        np = lthip_raw_pieces(d, len);
    }
    runs.pieces[i] = np;
}

// ---- the carry in place: behind k_restore_carry_runs.  A run whose source is its destination is KEPT and loses its pieces (a run is all
// kept or all moved: the distance from source to destination is constant over it).  A moved run goes through the caller's scratch: it
// gets the 16-byte units of its slot there and the pieces of its way IN (a slot starts on a 16-byte boundary); `pieces` stays what its
// way back OUT needs. ----
__global__ void k_restore_in_place_classify(uint32_t n, RunTables runs)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint32_t in = 0, u = 0;
    if (runs.pieces[i])
    {
        if (runs.src[i] == runs.dst[i])
            runs.pieces[i] = 0u;
        else
        {
            const uint64_t len = runs.len[i];
            in = lthip_raw_pieces(0, len);
            u = (uint32_t)((len + 15u) >> 4); // (the moved bytes and their padding stay below 2^36: lthip_restore_carry_in_place)
        }
    }
    runs.pieces_in[i] = in;
    runs.units[i] = u;
}

// first_unit = the exclusive scan of the units: where every run's slot starts in the scratch
__global__ void k_restore_in_place_slots(uint32_t n, RunTables runs)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        runs.slot[i] = (uint64_t)runs.first_unit[i] << 4;
}

// ---- a delivered image against the StoreIndex: one wave per image.  The header's dwords come through `Words`: AlignedWords for the
// images of lthip_restore_blocks, AnyWords for an image at any byte position (an archive's body) ----
struct AlignedWords
{
    const uint32_t* w;
    __device__ __forceinline__ explicit AlignedWords(const uint8_t* image) : w(reinterpret_cast<const uint32_t*>(image)) {} // 8-byte aligned by contract
    __device__ __forceinline__ uint32_t operator[](uint64_t j) const { return w[j]; }
};
// dword j of an image that starts mis = address & 3 bytes into an aligned dword: assembled from the two aligned dwords around it
// (v_alignbit, as k_copy.h does).  Both hold bytes of dword j, so no dword is read that holds no byte of the image: an image may end at
// the last byte of the allocation.
struct AnyWords
{
    const uint32_t* q;
    uint32_t sh;
    __device__ __forceinline__ explicit AnyWords(const uint8_t* image)
        : q(reinterpret_cast<const uint32_t*>(image - ((uintptr_t)image & 3u))), sh((uint32_t)((uintptr_t)image & 3u) * 8u)
    {
    }
    __device__ __forceinline__ uint32_t operator[](uint64_t j) const { return sh ? __builtin_amdgcn_alignbit(q[j + 1], q[j], sh) : q[j]; }
};

template <class Words>
__device__ __forceinline__ void check_image(const RItem* __restrict__ items, uint32_t k, const uint8_t* __restrict__ images, const StoreView& sv,
                                            uint32_t hash_identifier, uint32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x;
    if (i >= k)
        return;
    const uint32_t lane = threadIdx.x;
    const RItem it = items[i];
    const uint32_t b = it.block, n = sv.bcnt[b], tag = sv.btag[b], c0 = sv.bcoff[b], raw = sv.braw[b];
    const uint64_t hdr = 20ull + 12ull * n + (tag ? 8u : 0u);
    uint32_t st = 0;
    if ((uint64_t)it.size < hdr) // (nothing of it is read)
        st = LTHIP_RESTORE_BAD_HEADER;
    else
    {
        const Words w(images + it.image);
        bool bad = false;
        if (lane == 0)
        {
            const uint64_t h = sv.bhash[b];
            bad = w[0] != (uint32_t)h || w[1] != (uint32_t)(h >> 32) || w[2] != hash_identifier || w[3] != n || w[4] != tag;
            if (tag) // [raw size][compressed size] behind the BlockIndex
                bad = bad || w[5ull + 3ull * n] != raw || (uint64_t)w[6ull + 3ull * n] != (uint64_t)it.size - hdr;
        }
        for (uint32_t j = lane; j < n; j += 64)
        {
            const uint64_t h = sv.chash[c0 + j];
            bad = bad || w[5ull + 2ull * j] != (uint32_t)h || w[6ull + 2ull * j] != (uint32_t)(h >> 32) || w[5ull + 2ull * n + j] != sv.csize[c0 + j];
        }
        if (__builtin_amdgcn_ballot_w64(bad))
            st = LTHIP_RESTORE_BAD_HEADER;
        else if (!tag && (uint64_t)it.size != hdr + raw) // a raw image is its BlockIndex and its chunks, no more and no less
            st = LTHIP_RESTORE_BAD_PAYLOAD;
    }
    if (lane == 0)
        status[b] = st;
}

__global__ __launch_bounds__(64) void k_restore_check_images(const RItem* __restrict__ items, uint32_t k, const uint8_t* __restrict__ images,
                                                             StoreView sv, uint32_t hash_identifier, uint32_t* __restrict__ status)
{
    check_image<AlignedWords>(items, k, images, sv, hash_identifier, status);
}

__global__ __launch_bounds__(64) void k_restore_check_images_any(const RItem* __restrict__ items, uint32_t k, const uint8_t* __restrict__ images,
                                                                 StoreView sv, uint32_t hash_identifier, uint32_t* __restrict__ status)
{
    check_image<AnyWords>(items, k, images, sv, hash_identifier, status);
}

// ---- behind the decoders: their verdict into the status word; with verify, the byte range of every chunk of the good blocks (a bad
// block's chunks become empty ranges at offset 0: nothing of it is read) ----
__global__ __launch_bounds__(64) void k_restore_ranges(const RItem* __restrict__ items, uint32_t k, const uint32_t* __restrict__ outsz,
                                                       StoreView sv, uint32_t* __restrict__ status, uint32_t verify, uint64_t base, RangeView v)
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
    const uint32_t c0 = sv.bcoff[b], n = sv.bcnt[b];
    for (uint32_t j = lane; j < n; j += 64)
    {
        const uint32_t r = it.vfirst + j, c = c0 + j;
        v.off[r] = st ? 0ull : it.src - base + sv.coff[c];
        v.len[r] = st ? 0u : sv.csize[c];
        v.block[r] = b;
        v.chunk[r] = c;
    }
}

__global__ void k_restore_compare(uint32_t n, RangeView v, const uint64_t* __restrict__ chash, uint32_t* status, Counters* counters)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n)
        return;
    const uint32_t b = v.block[r];
    // (the header and payload bits were final before this launch; only the chunk bit is set beside these reads)
    if (__hip_atomic_load(&status[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (LTHIP_RESTORE_BAD_HEADER | LTHIP_RESTORE_BAD_PAYLOAD))
        return;
    if (v.hash[r] != chash[v.chunk[r]])
    {
        atomicOr(&status[b], LTHIP_RESTORE_BAD_CHUNK);
        atomicAdd(&counters->block_chunks_bad, 1ull);
    }
}

// ---- the scatter: a workgroup per entry of the call's blocks, block-major, copied by lthip_wg_copy (k_copy.h): source and destination
// sit at any byte positions, and no dword is read that holds no byte of the entry ----
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
    const uint8_t* s = reinterpret_cast<const uint8_t*>(it.src) + en.x;
    uint8_t* d = out + ((uint64_t)en.z | ((uint64_t)en.w << 32));
    lthip_wg_copy<RT>(d, s, en.y, threadIdx.x);
}

// ---- a cache: behind k_restore_check_images, the payload of every good raw block that has a slot into that slot, in pieces of
// CACHE_PIECE bytes (grid: the call's undecoded items x pieces).  A block whose status word is not 0 is not read: status 0 says that the
// image is exactly its header and `raw` bytes.  slot_of[i] == 0: item i has no slot, or is decoded into it. ----
constexpr uint32_t CACHE_PIECE = 1u << 18;
__global__ __launch_bounds__(RT) void k_restore_cache_copy(const RItem* __restrict__ items, const uint64_t* __restrict__ slot_of,
                                                           const uint32_t* __restrict__ status)
{
    const uint64_t to = slot_of[blockIdx.x];
    if (!to)
        return;
    const RItem it = items[blockIdx.x];
    const uint64_t at = (uint64_t)blockIdx.y * CACHE_PIECE;
    if (at >= it.raw || status[it.block] != 0u)
        return;
    const uint64_t n = std::min<uint64_t>(CACHE_PIECE, it.raw - at);
    lthip_wg_copy<RT>(reinterpret_cast<uint8_t*>(to + at), reinterpret_cast<const uint8_t*>(it.src + at), (uint32_t)n, threadIdx.x);
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

template <class T> int upload(lthip_ctx* ctx, T* d_dst, const std::vector<T>& h_src) { return upload(ctx, d_dst, h_src.data(), h_src.size() * sizeof(T)); }

using restore_call::round64;

// one kernel launch on the context's stream, timed as `kid`
template <class K, class... A> int launch(lthip_ctx* ctx, int kid, K kernel, dim3 grid, dim3 block, A... args)
{
    LaunchTimer tm(ctx, kid);
    hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, args...);
    LTHIP_LAUNCH_CHECK(ctx);
    return 0;
}

} // namespace

struct lthip_block_cache
{
    lthip_ctx* ctx;
    void* arena;
    block_cache::Table table;
    uint64_t slot_address(uint32_t s) const { return (uint64_t)(uintptr_t)arena + (uint64_t)s * table.slot_bytes(); }
};

// the base: its distinct chunks, what of the plan it feeds (the read-back of create), whether carry has queued it, the buffer of a carry in place
struct BaseState
{
    bool has_base = false, carried = false, in_place = false;
    uint32_t nub = 0, ncarry = 0, nmarked = 0, base_max_chunk = 0;
    uint64_t base_window = 0, carry_bytes = 0, carry_leaves = 0, moved_occ = 0, moved_bytes = 0;
    void* in_place_buf = nullptr;
    BaseView base;
    CarryView carry;
    RangeView base_ranges; // verify: the base chunks that feed something
};

// the cache (null: none attached).  A block with Blocks::fed is cache-fed from slot cslot[b]; reserved: the delivered blocks that have a
// reserved slot cslot[b], until finish commits or releases them
struct CacheLink
{
    lthip_block_cache* cache = nullptr;
    bool from_cache_done = false, pins_held = false;
    std::vector<uint64_t> bdigest, slot_of;
    std::vector<uint32_t> cslot, fed_blocks, reserved;
    uint64_t fed_bytes = 0, fed_entries = 0, c_inserted = 0, c_bypassed = 0, c_dropped = 0;
    void* d_cmem = nullptr;
    RItem* d_fed_items = nullptr;
    uint32_t* d_fed_outsz = nullptr;
    uint64_t* d_slot_of = nullptr;
    block_cache::Key cache_key(uint32_t hash_identifier, const restore_plan::StoreTables& st, uint32_t b) const { return {hash_identifier, st.bhash[b]}; }
    block_cache::Meta cache_meta(const restore_plan::StoreTables& st, uint32_t b) const { return block_cache::Meta{st.bcnt[b], st.braw[b], bdigest[b]}; }
    size_t carve_cache(Carver c, size_t nb)
    {
        c.take(&d_fed_items, fed_blocks.size()), c.take(&d_fed_outsz, fed_blocks.size()), c.take(&d_slot_of, nb);
        return c.at;
    }
    // gives back what the session holds of the cache: the slots it reserved and has not committed, and (pins) its pins
    void release_cache(bool pins)
    {
        if (!cache)
            return;
        for (const uint32_t b : reserved)
            cache->table.abort(cslot[b], false);
        reserved.clear();
        if (pins && pins_held)
        {
            for (const uint32_t b : fed_blocks)
                cache->table.unpin(cslot[b]);
            pins_held = false;
        }
    }
};

// host tables of a blocks call, kept for their capacity
struct CallTables
{
    restore_call::Call c;
    std::vector<RItem> items;
    std::vector<uint32_t> outsz, c_size, c_cap;
    std::vector<uint64_t> c_src, c_dst;
};

struct lthip_restore
{
    lthip_ctx* ctx = nullptr;
    uint32_t verify = 0, hash_identifier = 0;
    uint32_t nb = 0, m = 0, nocc = 0, max_chunk = 0;
    uint64_t block_chunks = 0; // the blocks' chunk counts summed: m for an index whose blocks share no chunk position
    uint64_t assets_selected = 0, out_bytes = 0;
    bool finished = false, blocks_queued = false; // blocks_queued: a call has queued work (an in-place carry and a cache come before that)
    restore_call::Blocks blk;                     // the StoreIndex and the plan on the host, and what was delivered
    std::vector<uint64_t> bbytes;                 // per block: the bytes its entries write ...
    std::vector<uint32_t> status;                 // ... and its status word, read back by finish
    BaseState bs;
    CacheLink cl;
    CallTables call;
    // the device side: one allocation for what lives as long as the session, one for what only the plan needs (PlanTmp)
    lthip_seen *seen = nullptr, *seen_base = nullptr;
    void *d_mem = nullptr, *d_tmp = nullptr;
    StoreView sv;
    uint32_t *d_status = nullptr, *d_firsts = nullptr, *d_outsz = nullptr;
    uint4* d_entries = nullptr;
    RItem* d_items = nullptr;
    Counters* d_counters = nullptr;
    RangeView ranges; // verify: the chunks of a blocks call

    size_t carve(Carver c, size_t items_cap)
    {
        const size_t nub = bs.nub;
        c.take(&sv.chash, m), c.take(&sv.csize, m), c.take(&sv.cblock, m), c.take(&sv.coff, m);
        c.take(&sv.bhash, nb), c.take(&sv.bcoff, nb), c.take(&sv.bcnt, nb), c.take(&sv.btag, nb), c.take(&sv.braw, nb), c.take(&d_status, nb);
        c.take(&d_firsts, (size_t)nb + 1), c.take(&d_entries, nocc), c.take(&d_items, items_cap), c.take(&d_outsz, items_cap), c.take(&d_counters, 1);
        if (verify)
            c.take(&ranges.off, block_chunks), c.take(&ranges.hash, block_chunks), c.take(&ranges.len, block_chunks),
                c.take(&ranges.block, block_chunks), c.take(&ranges.chunk, block_chunks);
        if (bs.has_base)
            c.take(&bs.carry.src, nocc), c.take(&bs.carry.dst, nocc), c.take(&bs.carry.len, nocc), c.take(&bs.carry.chunk, nocc),
                c.take(&bs.base.hash, nub), c.take(&bs.base.off, nub), c.take(&bs.base.size, nub), c.take(&bs.base.feed, nub), c.take(&bs.base.bad, nub);
        if (bs.has_base && verify)
            c.take(&bs.base_ranges.off, nub), c.take(&bs.base_ranges.hash, nub), c.take(&bs.base_ranges.len, nub), c.take(&bs.base_ranges.chunk, nub);
        return c.at;
    }
};

// the entries of k items in launches of 2^23 (a launch holds fewer than 2^32 threads)
static int launch_scatter(const lthip_restore* r, const RItem* d_items, uint32_t k, uint64_t entries, const uint32_t* d_outsz, void* d_out)
{
    LaunchTimer tm(r->ctx, LTHIP_K_GATHER);
    constexpr uint64_t LAUNCH_ENTRIES = 1u << 23;
    for (uint64_t e0 = 0; e0 < entries; e0 += LAUNCH_ENTRIES)
        hipLaunchKernelGGL(k_restore_scatter, dim3((uint32_t)std::min(LAUNCH_ENTRIES, entries - e0)), dim3(RT), 0, r->ctx->stream, d_items, k,
                           (const uint4*)r->d_entries, (const uint32_t*)r->d_status, d_outsz, (uint32_t)e0, (uint8_t*)d_out);
    LTHIP_LAUNCH_CHECK(r->ctx);
    return 0;
}

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
    if (r->d_mem || r->d_tmp || r->cl.d_cmem)
        (void)hipStreamSynchronize(r->ctx->stream);
    r->cl.release_cache(true); // (behind the wait: nothing of this session reads or writes a slot any more)
    lthip_seen_destroy(r->seen);
    lthip_seen_destroy(r->seen_base);
    if (r->cl.d_cmem)
        (void)hipFree(r->cl.d_cmem);
    if (r->d_mem)
        (void)hipFree(r->d_mem);
    if (r->d_tmp)
        (void)hipFree(r->d_tmp);
    delete r;
}

// What a session writes: byte windows of assets (lthip_restore_create_windows), or whole assets at asset_offsets -- which become one
// window per selected asset once the VersionIndex has been read --, or (list) occurrences that lie on the device already: no
// VersionIndex is read, and every occurrence is its whole chunk (lthip_restore_create_occurrences, the repack session).
struct Wanted
{
    const char* who;
    const uint64_t* asset_offsets;
    bool by_window;
    uint64_t window_count;
    const restore_windows::Window* windows;
    const lthip_occurrence_list* list = nullptr;
};

// `base` is optional: lthip_restore_create passes none, and then every step that serves it is skipped
static int restore_build(lthip_restore* r, const lthip_restore_config* cfg, const lthip_restore_base* base, const void* version_index,
                         size_t vi_size, const void* store_index, size_t si_size, const Wanted& wanted, uint64_t out_bytes)
{
    lthip_ctx* ctx = r->ctx;
    restore_parse::VersionIndex vi, bvi;
    restore_parse::StoreIndex si;
    if (!wanted.list && restore_parse::parse_version_index(version_index, vi_size, &vi))
        return lthip_fail(ctx, EBADF, "lthip_restore_create", "malformed version index");
    if (wanted.list)
        vi.hash_identifier = wanted.list->hash_identifier;
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
    const char* why = "";
    int refused;
    // ---- the base: per distinct chunk the offset of its first occurrence in a resident asset ----
    restore_plan::BaseTable bt;
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
        r->bs.has_base = true;
        r->bs.base_window = base->base_bytes;
        r->bs.nub = bvi.chunk_count;
        if ((refused = restore_plan::base_table(bvi, base->asset_offsets, base->base_bytes, &bt, &why)))
            return lthip_fail(ctx, refused, "lthip_restore_create_from_base", why);
        r->bs.base_max_chunk = bt.max_chunk;
    }
    // ---- the StoreIndex: per block its tables, per chunk position the block that holds it and where ----
    restore_plan::StoreTables& st = r->blk.st;
    if ((refused = restore_plan::store_tables(si, &st, &why)))
        return lthip_fail(ctx, refused, "lthip_restore_create", why);
    const uint32_t nb = r->nb = si.block_count, m = r->m = si.chunk_count, nub = r->bs.nub;
    r->max_chunk = st.max_chunk;
    r->block_chunks = st.block_chunks;
    // ---- occurrences: per window and chunk it touches (hash, full length, skip, clip, destination) ----
    restore_windows::Occurrences occ;
    if (wanted.list)
        refused = wanted.list->count > 0x7FFFFFFFull ? (why = "more than 2^31 - 1 occurrences", EINVAL) : 0;
    else if (wanted.by_window)
        refused = restore_windows::expand(vi, wanted.window_count, wanted.windows, out_bytes, &occ, &why);
    else
    {
        const std::vector<restore_windows::Window> whole = restore_plan::whole_asset_windows(vi, wanted.asset_offsets);
        refused = restore_windows::expand(vi, whole.size(), whole.data(), out_bytes, &occ, &why);
    }
    if (refused)
        return lthip_fail(ctx, refused, wanted.who, why);
    r->assets_selected = occ.assets_selected;
    const uint32_t nocc = r->nocc = wanted.list ? (uint32_t)wanted.list->count : (uint32_t)occ.hash.size();
    const bool clipped = !occ.clip.empty();
    // ---- device memory: the session's, and the plan's temporaries ----
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LTHIP_CHECK(ctx, lthip_hip_malloc(&r->d_mem, r->carve(Carver(), nb) + 256));
    r->carve(Carver(r->d_mem), nb);
    PlanTmp t;
    LTHIP_CHECK(ctx, lthip_hip_malloc(&r->d_tmp, t.carve(Carver(), nocc, nb, m, nub, clipped, base != nullptr) + 256));
    t.carve(Carver(r->d_tmp), nocc, nb, m, nub, clipped, base != nullptr);
    // ---- upload ----
    const StoreView& sv = r->sv;
    hipStream_t s = ctx->stream;
    int err;
    if ((err = upload(ctx, sv.chash, st.chash)) || (err = upload(ctx, sv.csize, st.csize)) || (err = upload(ctx, sv.cblock, st.cblock)) ||
        (err = upload(ctx, sv.coff, st.coff)) || (err = upload(ctx, sv.bhash, st.bhash)) || (err = upload(ctx, sv.bcoff, st.bcoff)) ||
        (err = upload(ctx, sv.bcnt, st.bcnt)) || (err = upload(ctx, sv.btag, st.btag)) || (err = upload(ctx, sv.braw, st.braw)))
        return err;
    if (!wanted.list && ((err = upload(ctx, t.ohash, occ.hash)) || (err = upload(ctx, t.occ.dst, occ.dst)) || (err = upload(ctx, t.occ.len, occ.len))))
        return err;
    if (wanted.list && nocc) // (the list lies on the device: queued on the stream that wrote it)
    {
        LTHIP_CHECK(ctx, hipMemcpyAsync(t.ohash, wanted.list->d_hash, (size_t)nocc * 8, hipMemcpyDeviceToDevice, ctx->stream));
        LTHIP_CHECK(ctx, hipMemcpyAsync(t.occ.dst, wanted.list->d_dst, (size_t)nocc * 8, hipMemcpyDeviceToDevice, ctx->stream));
        LTHIP_CHECK(ctx, hipMemcpyAsync(t.occ.len, wanted.list->d_len, (size_t)nocc * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (clipped && ((err = upload(ctx, t.occ.skip, occ.skip)) || (err = upload(ctx, t.occ.clip, occ.clip))))
        return err;
    if (base && ((err = upload(ctx, r->bs.base.hash, bt.hash)) || (err = upload(ctx, r->bs.base.off, bt.off)) ||
                 (err = upload(ctx, r->bs.base.size, bt.size))))
        return err;
    // (the staging ring has copied them: the host reads neither again, the rest of the StoreIndex stays)
    std::vector<uint32_t>().swap(st.cblock), std::vector<uint32_t>().swap(st.coff);
    r->blk.init();
    r->status.assign(nb, 0u), r->bbytes.assign(nb, 0ull);
    if (base && nub)
    {
        LTHIP_CHECK(ctx, hipMemsetAsync(r->bs.base.feed, 0, (size_t)nub * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(r->bs.base.bad, 0, (size_t)nub * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t.bmark, 0, (size_t)nub * 4, s));
    }
    LTHIP_CHECK(ctx, hipMemsetAsync(r->d_counters, 0, sizeof(Counters), s));
    if (nb)
    {
        LTHIP_CHECK(ctx, hipMemsetAsync(r->d_status, 0, (size_t)nb * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t.hist, 0, (size_t)nb * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t.cursor, 0, (size_t)nb * 4, s));
        LTHIP_CHECK(ctx, hipMemsetAsync(t.bbytes, 0, (size_t)nb * 8, s));
    }
    // ---- the plan: hash -> position in the StoreIndex's chunk list, occurrences per block, firsts, entries block-major ----
    if ((err = lthip_seen_create(ctx, m, &r->seen)) || (err = lthip_seen_add(r->seen, m, sv.chash, t.first, nullptr)))
        return err;
    // ... and, with a base, hash -> position among the base's chunks: an occurrence the base feeds is not resolved against the StoreIndex
    if (base)
    {
        if ((err = lthip_seen_create(ctx, nub, &r->seen_base)) || (err = lthip_seen_add(r->seen_base, nub, r->bs.base.hash, t.bfirst, nullptr)))
            return err;
        if (nocc && (err = lthip_seen_find(r->seen_base, nocc, t.ohash, t.occ.bpos)))
            return err;
    }
    if (nocc && ((err = lthip_seen_find(r->seen, nocc, t.ohash, t.occ.pos)) ||
                 (err = launch(ctx, LTHIP_K_OTHER, k_restore_resolve, dim3((nocc + 255u) / 256u), dim3(256), nocc, t, r->bs.base, sv, r->d_counters))))
        return err;
    if ((err = lthip_exclusive_scan_u32(ctx, t.hist, r->d_firsts, nb, nullptr, LTHIP_K_OTHER)))
        return err;
    if (base && ((err = lthip_exclusive_scan_u32(ctx, t.oflag, t.ofirst, nocc, nullptr, LTHIP_K_OTHER)) ||
                 (err = lthip_exclusive_scan_u32(ctx, t.bmark, t.mfirst, nub, nullptr, LTHIP_K_OTHER))))
        return err;
    if (nocc && (err = launch(ctx, LTHIP_K_OTHER, k_restore_fill, dim3((nocc + 255u) / 256u), dim3(256), nocc, t, r->bs.base, sv,
                              (const uint32_t*)r->d_firsts, r->d_entries, r->bs.carry, r->d_counters)))
        return err;
    if (base && r->verify && nub &&
        (err = launch(ctx, LTHIP_K_OTHER, k_restore_carry_marked, dim3((nub + 255u) / 256u), dim3(256), nub, t, r->bs.base, r->bs.base_ranges, r->d_counters)))
        return err;
    // ---- the one read-back: the firsts (and the bytes per block, for the statistics), what did not resolve, what the base feeds ----
    Counters counters = {};
    LTHIP_CHECK(ctx, hipMemcpyAsync(r->blk.firsts.data(), r->d_firsts, ((size_t)nb + 1) * 4, hipMemcpyDeviceToHost, s));
    if (nb)
        LTHIP_CHECK(ctx, hipMemcpyAsync(r->bbytes.data(), t.bbytes, (size_t)nb * 8, hipMemcpyDeviceToHost, s));
    LTHIP_CHECK(ctx, hipMemcpyAsync(&counters, r->d_counters, sizeof counters, hipMemcpyDeviceToHost, s));
    if (base)
    {
        LTHIP_CHECK(ctx, hipMemcpyAsync(&r->bs.ncarry, t.ofirst + nocc, 4, hipMemcpyDeviceToHost, s));
        LTHIP_CHECK(ctx, hipMemcpyAsync(&r->bs.nmarked, t.mfirst + nub, 4, hipMemcpyDeviceToHost, s));
    }
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    if (counters.unresolved)
        return lthip_fail(ctx, ENOENT, wanted.who,
                          base ? "a selected asset needs a chunk that neither the base nor the store index holds (or holds with another size)"
                               : "a selected asset or window needs a chunk the store index does not hold (or holds with another size)");
    r->bs.carry_bytes = counters.base_bytes;
    r->bs.carry_leaves = counters.base_verify_leaves;
    r->bs.moved_occ = counters.moved_occ;
    r->bs.moved_bytes = counters.moved_bytes;
    lthip_seen_destroy(r->seen_base);
    r->seen_base = nullptr;
    LTHIP_CHECK(ctx, hipFree(r->d_tmp));
    r->d_tmp = nullptr;
    for (uint32_t b = 0; b < nb; ++b)
        r->blk.needed += r->blk.is_needed(b);
    return 0;
}

static int restore_create(lthip_ctx* ctx, const lthip_restore_config* cfg, const lthip_restore_base* base, const void* version_index,
                          size_t vi_size, const void* store_index, size_t si_size, const Wanted& wanted, uint64_t out_bytes, lthip_restore** out)
{
    if (!ctx || !out || (!version_index && !wanted.list) || !store_index)
        return EINVAL;
    *out = nullptr;
    lthip_restore* r = new (std::nothrow) lthip_restore();
    if (!r)
        return ENOMEM;
    r->ctx = ctx;
    const int err = lthip_guarded(ctx, "lthip_restore_create",
                                  [&] { return restore_build(r, cfg, base, version_index, vi_size, store_index, si_size, wanted, out_bytes); });
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

// (lthip_internal.h) the session the repack session owns: its occurrences are the moved chunks, its output the work buffer
int lthip_restore_create_occurrences(lthip_ctx* ctx, const lthip_restore_config* cfg, const lthip_occurrence_list* list, const void* store_index,
                                     size_t si_size, uint64_t out_bytes, const char* who, lthip_restore** out)
{
    if (!list || (list->count && (!list->d_hash || !list->d_len || !list->d_dst)))
        return EINVAL;
    Wanted wanted{who, nullptr, false, 0, nullptr};
    wanted.list = list;
    return restore_create(ctx, cfg, nullptr, nullptr, 0, store_index, si_size, wanted, out_bytes, out);
}

uint64_t lthip_restore_outstanding(const lthip_restore* r) { return r->blk.needed - r->blk.needed_delivered; }

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
    *out_count = r->blk.needed;
    if (!block_hashes || capacity < r->blk.needed)
        return 0;
    uint64_t k = 0;
    for (uint32_t b = 0; b < r->nb; ++b)
        if (r->blk.is_needed(b))
            block_hashes[k++] = r->blk.st.bhash[b];
    return 0;
}

extern "C" size_t lthip_restore_scratch_bound(const lthip_restore* r, uint32_t block_count, const uint64_t* block_hashes)
{
    return r && (!block_count || block_hashes) ? (size_t)restore_call::scratch_bound(r->blk, block_count, block_hashes) : 0;
}

// ---- a blocks call in five stages: items and slots, check, decode, judge, scatter.  What the first hands to the others: ----
struct Queued
{
    size_t k = 0;                                            // the call's needed blocks: its items, group by group
    uint64_t slots = 0, entries = 0, ranges = 0, leaves = 0; // summed over the items: scratch handed out, entries, chunks and their leaves
    uint32_t copy_raw = 0;                                   // the largest raw block that is copied into a cache slot
};
// the lower of two addresses, a null one aside: the decoders and verify address everything they touch from one base
static uint64_t lowest(uint64_t a, uint64_t b) { return !a ? b : !b ? a : std::min(a, b); }

// Stage 1: an RItem per needed block.  A cache: every needed block reserves a slot when one is to be had; a tagged block is then decoded
// into it, a raw block copied.  Every other tagged block gets slot_bytes of the scratch.
static void queue_items(lthip_restore* r, const void* d_images, const uint64_t* image_offsets, const uint32_t* image_sizes, void* d_scratch, Queued* q)
{
    const restore_call::Blocks& blk = r->blk;
    CallTables& t = r->call;
    CacheLink& cl = r->cl;
    t.items.clear(), t.outsz.clear(), cl.slot_of.clear();
    for (const auto& group : t.c.group)
        for (const uint32_t i : group)
        {
            const uint32_t b = t.c.blocks[i];
            const bool tagged = blk.st.btag[b] != 0u;
            uint64_t in_cache = 0;
            if (cl.cache)
            {
                const uint32_t s = cl.cache->table.reserve(cl.cache_key(r->hash_identifier, blk.st, b), cl.cache_meta(blk.st, b));
                if (s == block_cache::NO_SLOT)
                    ++cl.c_bypassed;
                else
                {
                    cl.cslot[b] = s;
                    cl.reserved.push_back(b);
                    in_cache = cl.cache->slot_address(s);
                    if (!tagged)
                        q->copy_raw = std::max(q->copy_raw, blk.st.braw[b]);
                }
                cl.slot_of.push_back(tagged ? 0u : in_cache);
            }
            RItem it;
            it.image = image_offsets[i];
            it.src = !tagged    ? (uint64_t)(uintptr_t)d_images + image_offsets[i] + lthip_block_index_size(blk.st.bcnt[b])
                     : in_cache ? in_cache
                                : (uint64_t)(uintptr_t)d_scratch + q->slots;
            it.size = image_sizes[i];
            it.block = b;
            it.raw = blk.st.braw[b];
            it.efirst = (uint32_t)q->entries;
            it.ebase = blk.firsts[b];
            it.vfirst = (uint32_t)q->ranges;
            t.items.push_back(it);
            t.outsz.push_back(tagged ? NONE : it.raw); // (a decoder overwrites its blocks' words; a raw block has nothing to decode)
            if (!in_cache)
                q->slots += blk.slot_bytes(b);
            q->entries += blk.firsts[b + 1] - blk.firsts[b];
            q->ranges += blk.st.bcnt[b];
            q->leaves += blk.st.bleaves[b];
        }
    q->k = t.items.size();
}

// Stage 2: every image against the StoreIndex; behind it, with a cache, the raw blocks that have a slot into their slots
static int queue_check(lthip_restore* r, const void* d_images, const Queued& q, bool any_position)
{
    lthip_ctx* ctx = r->ctx;
    const size_t k = q.k, undecoded = r->call.c.group[0].size();
    int err;
    if ((err = upload(ctx, r->d_items, r->call.items.data(), k * sizeof(RItem))) || (err = upload(ctx, r->d_outsz, r->call.outsz.data(), k * 4)) ||
        (err = launch(ctx, LTHIP_K_OTHER, any_position ? k_restore_check_images_any : k_restore_check_images, dim3((uint32_t)k), dim3(64),
                      (const RItem*)r->d_items, (uint32_t)k, (const uint8_t*)d_images, r->sv, r->hash_identifier, r->d_status)))
        return err;
    if (!q.copy_raw)
        return 0;
    if ((err = upload(ctx, r->cl.d_slot_of, r->cl.slot_of.data(), undecoded * 8)))
        return err;
    return launch(ctx, LTHIP_K_GATHER, k_restore_cache_copy, dim3((uint32_t)undecoded, (q.copy_raw + CACHE_PIECE - 1u) / CACHE_PIECE), dim3(RT),
                  (const RItem*)r->d_items, (const uint64_t*)r->cl.d_slot_of, (const uint32_t*)r->d_status);
}

// Stage 3: one call per codec; sizes and places from the StoreIndex and the items alone.  dbase: what the destinations are relative to
static int queue_decode(lthip_restore* r, const void* d_images, uint64_t dbase)
{
    CallTables& t = r->call;
    size_t at = t.c.group[0].size();
    for (int g = 1; g < 3; ++g)
    {
        const size_t cnt = t.c.group[g].size();
        if (!cnt)
            continue;
        t.c_src.clear(), t.c_size.clear(), t.c_dst.clear(), t.c_cap.clear();
        for (size_t j = 0; j < cnt; ++j)
        {
            const RItem& it = t.items[at + j];
            const uint64_t hdr = lthip_stored_block_header_size(r->blk.st.bcnt[it.block]);
            t.c_src.push_back(it.image + hdr);
            t.c_size.push_back((uint32_t)(it.size - hdr));
            t.c_dst.push_back(it.src - dbase);
            t.c_cap.push_back(it.raw); // (a slot holds at least the raw size of the block that reserved it)
        }
        const int err = (g == 1 ? lthip_lz4_decompress_blocks : lthip_zstd_decompress_blocks)(
            r->ctx, d_images, (uint32_t)cnt, t.c_src.data(), t.c_size.data(), (void*)(uintptr_t)dbase, t.c_dst.data(), t.c_cap.data(), r->d_outsz + at);
        if (err)
            return err;
        at += cnt;
    }
    return 0;
}

// Stage 4: the decoders' verdict, then verify, both before anything is copied out.  base: what the ranges verify hashes are relative to
static int queue_judge(lthip_restore* r, uint64_t base, const Queued& q)
{
    lthip_ctx* ctx = r->ctx;
    int err = launch(ctx, LTHIP_K_OTHER, k_restore_ranges, dim3((uint32_t)q.k), dim3(64), (const RItem*)r->d_items, (uint32_t)q.k,
                     (const uint32_t*)r->d_outsz, r->sv, r->d_status, r->verify, base, r->ranges);
    if (err || !r->verify || !q.ranges)
        return err;
    if ((err = lthip_hash_ranges_by_id(ctx, r->hash_identifier, (const void*)(uintptr_t)base, q.ranges, r->ranges.off, r->ranges.len, r->max_chunk,
                                       q.leaves, r->ranges.hash)))
        return err;
    return launch(ctx, LTHIP_K_OTHER, k_restore_compare, dim3((uint32_t)((q.ranges + 255u) / 256u)), dim3(256), (uint32_t)q.ranges, r->ranges,
                  (const uint64_t*)r->sv.chash, r->d_status, r->d_counters);
}

// The accepted call r->call.c.  any_position: the images lie at any byte positions (an archive's body), k_restore_check_images_any checks them
static int restore_queue(lthip_restore* r, const void* d_images, const uint64_t* image_offsets, const uint32_t* image_sizes, void* d_scratch,
                         void* d_out, bool any_position)
{
    restore_call::commit(&r->blk, &r->call.c, image_sizes);
    r->finished = false;
    Queued q;
    queue_items(r, d_images, image_offsets, image_sizes, d_scratch, &q);
    if (!q.k)
        return 0;
    r->blocks_queued = true;
    LTHIP_CHECK(r->ctx, hipSetDevice(r->ctx->device));
    // the decoders take one destination base: the scratch, with a cache the lower of the scratch and the arena; verify reads the raw
    // blocks where they lie in the images as well
    const uint64_t dbase = lowest((uint64_t)(uintptr_t)d_scratch, r->cl.cache ? (uint64_t)(uintptr_t)r->cl.cache->arena : 0u);
    const uint64_t base = lowest((uint64_t)(uintptr_t)d_images, r->cl.cache || q.slots ? dbase : 0u);
    int err;
    if ((err = queue_check(r, d_images, q, any_position)) || (err = queue_decode(r, d_images, dbase)) || (err = queue_judge(r, base, q)))
        return err;
    return launch_scatter(r, r->d_items, (uint32_t)q.k, q.entries, r->d_outsz, d_out);
}

// lthip_restore_blocks (its hashes; any_position false: an image offset that is not 8-byte aligned is refused) and
// lthip_restore_archive_blocks (the block indices its pick gave): the refusals, before anything is queued or changed, then the call
static int restore_deliver(lthip_restore* r, uint32_t block_count, const uint64_t* block_hashes, const uint32_t* blocks, const void* d_images,
                           const uint64_t* image_offsets, const uint32_t* image_sizes, void* d_scratch, uint64_t scratch_bytes, void* d_out,
                           bool any_position, const char* who)
{
    int refused = 0;
    const int err = lthip_guarded(r->ctx, who, [&] {
        const restore_call::Where w{d_scratch, d_out, r->bs.in_place_buf, scratch_bytes, any_position};
        refused = restore_call::resolve(r->blk, block_count, block_hashes, blocks, image_offsets, w, &r->call.c);
        return refused ? 0 : restore_queue(r, d_images, image_offsets, image_sizes, d_scratch, d_out, any_position);
    });
    if (refused)
        return lthip_fail(r->ctx, refused, who, r->call.c.why);
    if (err) // (a call that did not queue all of its work commits nothing: no status word of it can be trusted)
        r->cl.release_cache(false);
    return err;
}

extern "C" int lthip_restore_blocks(lthip_restore* r, uint32_t block_count, const uint64_t* block_hashes, const void* d_images,
                                    const uint64_t* image_offsets, const uint32_t* image_sizes, void* d_scratch, uint64_t scratch_bytes, void* d_out)
{
    if (!r || (block_count && (!block_hashes || !d_images || !image_offsets || !image_sizes)))
        return EINVAL;
    return restore_deliver(r, block_count, block_hashes, nullptr, d_images, image_offsets, image_sizes, d_scratch, scratch_bytes, d_out, false,
                           "lthip_restore_blocks");
}

// ---- fed from an archive's body (archive_layout.h; the pick: restore_call.h) ----
extern "C" size_t lthip_restore_archive_scratch_bound(const lthip_restore* r, const lthip_archive* archive, uint64_t window_first_byte,
                                                      uint64_t window_bytes)
{
    restore_call::Pick p;
    if (!r || !archive || lthip_guarded(nullptr, nullptr, [&] { return restore_call::pick(r->blk, archive->a, window_first_byte, window_bytes, &p), 0; }))
        return 0;
    return (size_t)p.scratch;
}

extern "C" int lthip_restore_archive_blocks(lthip_restore* r, const lthip_archive* archive, const void* d_window, uint64_t window_first_byte,
                                            uint64_t window_bytes, void* d_scratch, uint64_t scratch_bytes, void* d_out, uint32_t* delivered,
                                            uint64_t* next_byte)
{
    if (!r || !archive || !delivered || !next_byte)
        return EINVAL;
    *delivered = 0;
    return lthip_guarded(r->ctx, "lthip_restore_archive_blocks", [&] {
        restore_call::Pick p;
        restore_call::pick(r->blk, archive->a, window_first_byte, window_bytes, &p);
        *next_byte = p.next_byte;
        const uint32_t k = (uint32_t)p.blocks.size();
        if (!k)
            return 0;
        if (!d_window)
            return lthip_fail(r->ctx, EINVAL, "lthip_restore_archive_blocks", "null window");
        const int err = restore_deliver(r, k, nullptr, p.blocks.data(), d_window, p.offsets.data(), p.sizes.data(), d_scratch, scratch_bytes, d_out,
                                        true, "lthip_restore_archive_blocks");
        if (err) // (refused, or not all queued: the lowest outstanding block may be one of this window's)
        {
            for (const uint64_t o : p.offsets)
                *next_byte = std::min(*next_byte, window_first_byte + o);
            return err;
        }
        *delivered = k;
        return 0;
    });
}

extern "C" int lthip_restore_archive_ranges(const lthip_restore* r, const lthip_archive* archive, uint64_t max_gap, uint64_t* ranges, uint64_t capacity,
                                            uint64_t* count)
{
    if (!r || !archive || !count)
        return EINVAL;
    return lthip_guarded(nullptr, nullptr, [&] {
        restore_call::Pick p;
        restore_call::pick(r->blk, archive->a, 0, ~0ull, &p); // every needed, outstanding block
        std::vector<std::pair<uint64_t, uint64_t>> v;
        for (size_t i = 0; i < p.blocks.size(); ++i)
            v.emplace_back(p.offsets[i], (uint64_t)p.sizes[i]);
        archive_layout::merge_ranges(&v, max_gap);
        *count = v.size();
        if (!ranges || capacity < v.size())
            return 0;
        for (size_t i = 0; i < v.size(); ++i)
            ranges[2 * i] = v[i].first, ranges[2 * i + 1] = v[i].second;
        return 0;
    });
}

// d_scratch == null: out of place, d_base -> d_out.  Otherwise in place: d_base == d_out is the one buffer, and the moved runs go through
// d_scratch (16-byte aligned, lthip_restore_in_place_scratch_bound), all reads before all writes.
static int carry_queue(lthip_restore* r, const void* d_base, void* d_out, void* d_scratch)
{
    lthip_ctx* ctx = r->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint32_t n = r->bs.ncarry;
    const bool in_place = r->bs.in_place;
    int err;
    // ---- verify: the base chunks that feed something, hashed where they lie, before anything of them is copied ----
    const uint32_t* bbad = nullptr;
    if (r->verify && r->bs.nmarked)
    {
        const BaseState& bs = r->bs;
        if ((err = lthip_hash_ranges_by_id(ctx, r->hash_identifier, d_base, bs.nmarked, bs.base_ranges.off, bs.base_ranges.len, bs.base_max_chunk,
                                           bs.carry_leaves, bs.base_ranges.hash)) ||
            (err = launch(ctx, LTHIP_K_OTHER, k_restore_carry_compare, dim3((bs.nmarked + 255u) / 256u), dim3(256), bs.nmarked, bs.base_ranges, bs.base,
                          r->d_counters)))
            return err;
        bbad = r->bs.base.bad;
    }
    if (in_place && !r->bs.moved_occ) // everything the base feeds lies where it belongs: no copy is queued
        return 0;
    RunTables runs;
    void* tab = nullptr;
    if ((err = lthip_scratch(ctx, S_CARRY_RUNS, runs.carve(Carver(), n, in_place), &tab)))
        return err;
    runs.carve(Carver(tab), n, in_place);
    // ---- runs: boundaries, their scan, a slot per entry that starts a run, the pieces' scan, the copy ----
    const dim3 grid((n + 255u) / 256u), block(256);
    if ((err = launch(ctx, LTHIP_K_GATHER, k_restore_carry_bounds, grid, block, n, r->bs.carry, bbad, runs)) ||
        (err = lthip_exclusive_scan_u32(ctx, runs.bound, runs.rank, n, nullptr, LTHIP_K_GATHER)) ||
        (err = launch(ctx, LTHIP_K_GATHER, k_restore_carry_runs, grid, block, n, r->bs.carry, bbad, runs)))
        return err;
    if (!in_place)
    {
        if ((err = lthip_exclusive_scan_u32(ctx, runs.pieces, runs.first_piece, n, nullptr, LTHIP_K_GATHER)))
            return err;
        return lthip_raw_copy_runs(ctx, runs.first_piece, n, runs.src, runs.dst, runs.len, d_base, d_out,
                                   r->bs.carry_bytes / (LTHIP_RAW_PIECE_VEC * 16u) + n);
    }
    // ---- in place: kept runs drop out, moved runs get a slot; pass 1 buffer -> scratch, pass 2 scratch -> buffer ----
    if ((err = launch(ctx, LTHIP_K_GATHER, k_restore_in_place_classify, grid, block, n, runs)) ||
        (err = lthip_exclusive_scan_u32(ctx, runs.units, runs.first_unit, n, nullptr, LTHIP_K_GATHER)) ||
        (err = lthip_exclusive_scan_u32(ctx, runs.pieces_in, runs.first_piece_in, n, nullptr, LTHIP_K_GATHER)) ||
        (err = lthip_exclusive_scan_u32(ctx, runs.pieces, runs.first_piece, n, nullptr, LTHIP_K_GATHER)) ||
        (err = launch(ctx, LTHIP_K_GATHER, k_restore_in_place_slots, grid, block, n, runs)))
        return err;
    const uint64_t pieces_bound = r->bs.moved_bytes / (LTHIP_RAW_PIECE_VEC * 16u) + r->bs.moved_occ;
    if ((err = lthip_raw_copy_runs(ctx, runs.first_piece_in, n, runs.src, runs.slot, runs.len, d_base, d_scratch, pieces_bound)))
        return err;
    return lthip_raw_copy_runs(ctx, runs.first_piece, n, runs.slot, runs.dst, runs.len, d_scratch, d_out, pieces_bound);
}

extern "C" int lthip_restore_carry(lthip_restore* r, const void* d_base, void* d_out)
{
    if (!r)
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    // ---- the refusals, before anything is queued or changed ----
    if (!r->bs.has_base)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry", "the session was created without a base");
    if (r->bs.carried)
        return lthip_fail(ctx, EEXIST, "lthip_restore_carry", "the base was carried before");
    if (r->bs.ncarry)
    {
        if (!d_base || !d_out)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry", "null base or output");
        const uint64_t b0 = (uint64_t)(uintptr_t)d_base, o0 = (uint64_t)(uintptr_t)d_out;
        if (b0 < o0 + r->out_bytes && o0 < b0 + r->bs.base_window)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry", "the base and the output overlap: the update is out of place");
        const int err = carry_queue(r, d_base, d_out, nullptr);
        if (err)
            return err;
    }
    r->bs.carried = true;
    r->finished = false;
    return 0;
}

// what the moved runs need in the caller's scratch: their bytes, every run's slot rounded up to 16 bytes (a run holds at least one moved
// occurrence), and room to start the first slot on a 16-byte boundary
static uint64_t in_place_bound(const lthip_restore* r) { return r->bs.moved_occ ? r->bs.moved_bytes + 16u * r->bs.moved_occ + 64u : 0u; }

extern "C" size_t lthip_restore_in_place_scratch_bound(const lthip_restore* r) { return r && r->bs.has_base ? (size_t)in_place_bound(r) : 0; }

extern "C" int lthip_restore_in_place_stats(const lthip_restore* r, uint64_t out[4])
{
    if (!r || !out)
        return EINVAL;
    out[0] = r->bs.has_base ? r->bs.ncarry - r->bs.moved_occ : 0u;
    out[1] = r->bs.has_base ? r->bs.carry_bytes - r->bs.moved_bytes : 0u;
    out[2] = r->bs.has_base ? r->bs.moved_occ : 0u;
    out[3] = r->bs.has_base ? r->bs.moved_bytes : 0u;
    return 0;
}

extern "C" int lthip_restore_carry_in_place(lthip_restore* r, void* d_buf, void* d_scratch, uint64_t scratch_bytes)
{
    if (!r)
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    // ---- the refusals, before anything is queued or changed ----
    if (!r->bs.has_base)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "the session was created without a base");
    if (r->bs.carried)
        return lthip_fail(ctx, EEXIST, "lthip_restore_carry_in_place", "the base was carried before");
    if (r->blocks_queued)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "a blocks call has queued work: the carry in place comes first");
    if (r->bs.ncarry && !d_buf)
        return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "null buffer");
    void* scratch = nullptr;
    if (r->bs.moved_occ)
    {
        const uint64_t bound = in_place_bound(r);
        if (bound >> 36) // (the slots are placed by a 32-bit scan of 16-byte units)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "more than 64 GiB would move: update out of place");
        if (!d_scratch)
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "null scratch");
        const uint64_t b0 = (uint64_t)(uintptr_t)d_buf, s0 = (uint64_t)(uintptr_t)d_scratch;
        if (s0 < b0 + std::max(r->bs.base_window, r->out_bytes) && b0 < s0 + std::max(bound, scratch_bytes))
            return lthip_fail(ctx, EINVAL, "lthip_restore_carry_in_place", "the scratch overlaps the buffer");
        if (scratch_bytes < bound)
            return lthip_fail(ctx, ENOMEM, "lthip_restore_carry_in_place", "scratch below lthip_restore_in_place_scratch_bound");
        scratch = (void*)(uintptr_t)((s0 + 15u) & ~(uint64_t)15u);
    }
    r->bs.in_place = true;
    const int err = r->bs.ncarry ? carry_queue(r, d_buf, d_buf, scratch) : 0;
    if (err)
    {
        r->bs.in_place = false;
        return err;
    }
    r->bs.in_place_buf = d_buf;
    r->bs.carried = true;
    r->finished = false;
    return 0;
}

extern "C" int lthip_restore_layout_in_place(const void* base_vi, size_t base_vi_size, const uint64_t* base_offsets, uint64_t base_bytes,
                                             const void* target_vi, size_t target_vi_size, uint64_t align, uint64_t* target_offsets,
                                             uint32_t* asset_count, uint64_t* total_bytes, uint32_t* kept_assets)
{
    return lthip_guarded(nullptr, nullptr, [&] {
        return restore_layout::in_place(base_vi, base_vi_size, base_offsets, base_bytes, target_vi, target_vi_size, align, target_offsets, asset_count,
                                        total_bytes, kept_assets);
    });
}

extern "C" int lthip_version_diff(const void* source_vi, size_t source_size, const void* target_vi, size_t target_size, uint32_t* source_removed,
                                  uint32_t* target_added, uint32_t* source_content_modified, uint32_t* target_content_modified,
                                  uint32_t* source_permissions_modified, uint32_t* target_permissions_modified, uint32_t counts[4])
{
    if (!source_vi || !target_vi || !counts)
        return EINVAL;
    return lthip_guarded(nullptr, nullptr, [&] {
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
    });
}

extern "C" int lthip_restore_finish(lthip_restore* r, lthip_restore_result* out)
{
    if (!r || (out && (out->struct_size < 16 || out->struct_size > 4096)))
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    Counters counters = {};
    if (r->nb)
        LTHIP_CHECK(ctx, hipMemcpyAsync(r->status.data(), r->d_status, (size_t)r->nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    LTHIP_CHECK(ctx, hipMemcpyAsync(&counters, r->d_counters, sizeof counters, hipMemcpyDeviceToHost, ctx->stream));
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    r->finished = true;
    lthip_restore_result res;
    memset(&res, 0, sizeof res);
    res.assets_selected = r->assets_selected;
    res.occurrences = r->nocc;
    res.blocks_needed = r->blk.needed;
    res.blocks_delivered = r->blk.delivered_all;
    res.blocks_unneeded = r->blk.unneeded;
    res.chunks_mismatched = counters.block_chunks_bad;
    res.base_occurrences = r->bs.ncarry;
    res.base_bytes = r->bs.carry_bytes;
    res.base_chunks_mismatched = counters.base_chunks_bad;
    if (r->bs.carried) // (what a mismatched base chunk would have fed was left out of the runs)
    {
        res.occurrences_written = r->bs.ncarry - counters.base_bad_occ;
        res.bytes_written = r->bs.carry_bytes - counters.base_bad_bytes;
    }
    const auto wrote = [&](uint32_t b) { res.occurrences_written += r->blk.firsts[b + 1] - r->blk.firsts[b], res.bytes_written += r->bbytes[b]; };
    for (uint32_t b = 0; b < r->nb; ++b)
    {
        if (!r->blk.delivered[b] || !r->blk.is_needed(b))
            continue;
        if (r->status[b])
            ++res.blocks_bad;
        else
            wrote(b);
        if (r->blk.st.btag[b] != 0u && !(r->status[b] & (LTHIP_RESTORE_BAD_HEADER | LTHIP_RESTORE_BAD_PAYLOAD)))
            res.decoded_bytes += r->blk.st.braw[b];
    }
    if (r->cl.cache)
    {
        // the status words are final: a good block's reserved slot becomes an entry, every other one is given back
        block_cache::Table& table = r->cl.cache->table;
        for (const uint32_t b : r->cl.reserved)
        {
            if (r->status[b])
                table.abort(r->cl.cslot[b], true), ++r->cl.c_dropped;
            else if (table.commit(r->cl.cslot[b], r->verify != 0u))
                ++r->cl.c_inserted;
            else
                ++r->cl.c_bypassed;
        }
        r->cl.reserved.clear();
        if (r->cl.from_cache_done)
            for (const uint32_t b : r->cl.fed_blocks)
                wrote(b);
    }
    const bool outstanding =
        r->blk.needed_delivered < r->blk.needed || (r->bs.ncarry && !r->bs.carried) || (!r->cl.fed_blocks.empty() && !r->cl.from_cache_done);
    const int code = res.blocks_bad || res.base_chunks_mismatched ? EBADF : outstanding ? ENOENT : 0;
    if (!code)
        r->cl.release_cache(true); // (the session is complete: its pins go)
    if (out)
    {
        const uint64_t have = out->struct_size;
        res.struct_size = have < sizeof res ? have : sizeof res;
        memcpy(out, &res, (size_t)res.struct_size);
    }
    return code;
}

// ---- the cache of decoded blocks ----
extern "C" int lthip_block_cache_create(lthip_ctx* ctx, uint32_t slot_count, uint64_t slot_bytes, lthip_block_cache** out)
{
    if (out)
        *out = nullptr;
    if (!ctx || !out || !slot_count || !slot_bytes || slot_bytes > (1ull << 40))
        return EINVAL;
    const uint64_t bytes = round64(slot_bytes);
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    void* arena = nullptr;
    LTHIP_CHECK(ctx, lthip_hip_malloc(&arena, (size_t)(bytes * slot_count)));
    const int err = lthip_guarded(ctx, "lthip_block_cache_create",
                                  [&] { return *out = new lthip_block_cache{ctx, arena, block_cache::Table(slot_count, bytes)}, 0; });
    if (err)
        (void)hipFree(arena);
    return err;
}

extern "C" void lthip_block_cache_destroy(lthip_block_cache* c)
{
    if (!c)
        return;
    (void)hipSetDevice(c->ctx->device);
    (void)hipStreamSynchronize(c->ctx->stream);
    (void)hipFree(c->arena);
    delete c;
}

extern "C" int lthip_block_cache_contains(const lthip_block_cache* c, uint32_t hash_identifier, uint32_t count, const uint64_t* block_hashes,
                                          uint8_t* held)
{
    if (!c || (count && (!block_hashes || !held)))
        return EINVAL;
    for (uint32_t i = 0; i < count; ++i)
        held[i] = c->table.lookup(block_cache::Key{hash_identifier, block_hashes[i]}) != block_cache::NO_SLOT ? 1u : 0u;
    return 0;
}

extern "C" int lthip_block_cache_clear(lthip_block_cache* c)
{
    if (!c)
        return EINVAL;
    return c->table.clear() ? 0 : lthip_fail(c->ctx, EBUSY, "lthip_block_cache_clear", "an entry is pinned or a slot is reserved by a live session");
}

extern "C" int lthip_block_cache_stats(const lthip_block_cache* c, uint64_t out[10])
{
    if (!c || !out)
        return EINVAL;
    const block_cache::Counts& n = c->table.counts();
    const uint64_t v[10] = {c->table.slot_count(), c->table.slot_bytes(), c->table.resident(), c->table.pinned(), c->table.reserved(),
                            n.hits,                n.inserted,            n.evicted,           n.bypassed,        n.dropped};
    memcpy(out, v, sizeof v);
    return 0;
}

static int set_cache(lthip_restore* r, lthip_block_cache* c)
{
    lthip_ctx* ctx = r->ctx;
    const uint32_t nb = r->nb;
    const restore_plan::StoreTables& st = r->blk.st;
    // ---- which needed blocks the cache feeds: a visible entry with the same chunk count, raw size and chunk table (verify: verified) ----
    r->cl.bdigest.assign(nb, 0u), r->cl.cslot.assign(nb, block_cache::NO_SLOT);
    for (uint32_t b = 0; b < nb; ++b)
        if (r->blk.is_needed(b)) // (only a needed block is looked up, now or when it is delivered)
            r->cl.bdigest[b] = block_cache::table_digest(st.chash.data() + st.bcoff[b], st.csize.data() + st.bcoff[b], st.bcnt[b]);
    std::vector<RItem> items;
    std::vector<uint32_t> outsz;
    uint64_t entries = 0, bytes = 0;
    for (uint32_t b = 0; b < nb; ++b)
    {
        if (!r->blk.is_needed(b))
            continue;
        const uint32_t s = c->table.lookup(r->cl.cache_key(r->hash_identifier, st, b));
        if (s == block_cache::NO_SLOT || !c->table.matches(s, r->cl.cache_meta(st, b), r->verify != 0u))
            continue;
        r->cl.cslot[b] = s;
        r->cl.fed_blocks.push_back(b);
        RItem it = {};
        it.src = c->slot_address(s);
        it.block = b;
        it.raw = st.braw[b];
        it.efirst = (uint32_t)entries;
        it.ebase = r->blk.firsts[b];
        items.push_back(it);
        outsz.push_back(it.raw);
        entries += r->blk.firsts[b + 1] - r->blk.firsts[b];
        bytes += it.raw;
    }
    // ---- the session's device tables for the cache; on an error the session stays as it was ----
    int err = 0;
    if (hipSetDevice(ctx->device) != hipSuccess)
        err = lthip_fail(ctx, EIO, "lthip_restore_set_cache", "hipSetDevice");
    else if (lthip_hip_malloc(&r->cl.d_cmem, r->cl.carve_cache(Carver(), nb) + 256) != hipSuccess)
        err = lthip_fail(ctx, ENOMEM, "lthip_restore_set_cache", "device tables");
    if (!err)
    {
        r->cl.carve_cache(Carver(r->cl.d_cmem), nb);
        if (!items.empty() && !(err = upload(ctx, r->cl.d_fed_items, items)))
            err = upload(ctx, r->cl.d_fed_outsz, outsz);
    }
    if (err)
    {
        if (r->cl.d_cmem)
        {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(r->cl.d_cmem);
        }
        r->cl.d_cmem = nullptr;
        return err;
    }
    for (const uint32_t b : r->cl.fed_blocks)
    {
        c->table.pin(r->cl.cslot[b]);
        r->blk.fed[b] = 1;
    }
    r->cl.pins_held = true;
    r->blk.needed -= r->cl.fed_blocks.size();
    r->cl.fed_entries = entries;
    r->cl.fed_bytes = bytes;
    r->cl.cache = c;
    return 0;
}

extern "C" int lthip_restore_set_cache(lthip_restore* r, lthip_block_cache* c)
{
    if (!r || !c)
        return EINVAL;
    if (c->ctx != r->ctx)
        return lthip_fail(r->ctx, EINVAL, "lthip_restore_set_cache", "the cache belongs to another context");
    if (r->cl.cache)
        return lthip_fail(r->ctx, EEXIST, "lthip_restore_set_cache", "the session has a cache");
    if (r->blocks_queued)
        return lthip_fail(r->ctx, EINVAL, "lthip_restore_set_cache", "a blocks call has queued work: the cache is attached before the first one");
    const int err = lthip_guarded(r->ctx, "lthip_restore_set_cache", [&] { return set_cache(r, c); });
    if (err) // (the session stays as it was)
        r->cl.fed_blocks.clear();
    return err;
}

extern "C" int lthip_restore_from_cache(lthip_restore* r, void* d_out)
{
    if (!r)
        return EINVAL;
    lthip_ctx* ctx = r->ctx;
    if (!r->cl.cache)
        return lthip_fail(ctx, EINVAL, "lthip_restore_from_cache", "the session has no cache");
    if (r->cl.from_cache_done)
        return lthip_fail(ctx, EEXIST, "lthip_restore_from_cache", "the cache-fed blocks were queued before");
    const uint32_t k = (uint32_t)r->cl.fed_blocks.size();
    if (k)
    {
        if (!d_out)
            return lthip_fail(ctx, EINVAL, "lthip_restore_from_cache", "null output");
        if (r->bs.in_place_buf && d_out != r->bs.in_place_buf)
            return lthip_fail(ctx, EINVAL, "lthip_restore_from_cache", "the base was carried in place: the output is that buffer");
        LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
        // (a cache-fed block is never delivered as needed: its status word stays 0)
        if (const int err = launch_scatter(r, r->cl.d_fed_items, k, r->cl.fed_entries, r->cl.d_fed_outsz, d_out))
            return err;
        r->blocks_queued = true;
        r->finished = false;
    }
    r->cl.from_cache_done = true;
    return 0;
}

extern "C" int lthip_restore_cache_stats(const lthip_restore* r, uint64_t out[6])
{
    if (!r || !out)
        return EINVAL;
    out[0] = r->cl.fed_blocks.size();
    out[1] = r->cl.fed_bytes;
    out[2] = r->cl.c_inserted;
    out[3] = r->cl.c_bypassed;
    out[4] = r->cl.c_dropped;
    out[5] = r->cl.from_cache_done ? r->cl.fed_entries : 0u;
    return 0;
}

extern "C" int lthip_restore_block_status(const lthip_restore* r, uint32_t count, const uint64_t* block_hashes, uint32_t* status)
{
    if (!r || (count && (!block_hashes || !status)))
        return EINVAL;
    if (!r->finished)
        return lthip_fail(r->ctx, EINVAL, "lthip_restore_block_status", "valid after lthip_restore_finish");
    for (uint32_t i = 0; i < count; ++i)
    {
        const uint32_t b = r->blk.find(block_hashes[i]);
        if (b == NONE)
            return lthip_fail(r->ctx, ENOENT, "lthip_restore_block_status", "a block hash the store index does not hold");
        status[i] = !r->blk.is_needed(b) ? 0u : !r->blk.delivered[b] ? LTHIP_RESTORE_NOT_DELIVERED : r->status[b];
    }
    return 0;
}
