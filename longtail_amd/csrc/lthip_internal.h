// lthip_internal.h -- shared declarations of liblongtail_hip.so (C++/HIP side, gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <new>
#include <vector>

#include "../../include/longtail_hip.h"

// ---------------------------------------------------------------------------------------------------
// device-side descriptors
// ---------------------------------------------------------------------------------------------------
struct PartDev
{
    uint64_t off;         // byte offset of the part in the data buffer (16-byte aligned)
    uint64_t size;        // bytes (< 2^32)
    uint64_t bm0_base;    // first 64-bit word of this part in the level-0 candidate bitmap (1 bit / byte)
    uint64_t bm1_base;    // first 64-bit word in the level-1 summary (1 bit / 64-byte run)
    uint64_t region_base; // first slot of this part in the bounded (rel_off,len) chunk region
    uint32_t tile_base;   // first buzhash tile of this part
    uint32_t region_cap;  // slots in the region
};

// The walking scan that hashes (k_buzhash_hash_walk) gives every part a run of slots for the chaining values of its leaves, sized by a
// bound of them: a leaf per chunk beyond ceil(size / 1024) at the most, and ceil(size / 1024) <= 16 tiles of 16 KiB.  So the runs need no
// field of their own: part p's starts at region_base + 16 tile_base, and a plan's take chunk_cap + 16 ntiles slots.
__host__ __device__ inline uint64_t lthip_part_run_base(const PartDev& p) { return p.region_base + 16ull * p.tile_base; }

// exact "H % d == d-1" test without a division:  d = dodd << k2 ;  inv = dodd^-1 mod 2^32
//   t = ror32(h*inv + addc, k2) <= qlim            (lthip_plan.cpp explains the derivation)
struct DivTest
{
    uint32_t d;
    uint32_t inv;
    uint32_t addc;
    uint32_t k2;
    uint32_t qlim;
    uint32_t pow2; // d is a power of two: test (h & (d-1)) == d-1 instead
};

// what the parts a plan is aimed at come to (plan_layout, lthip_ctx.hip): the launches are sized by these
struct PlanExtents
{
    uint32_t nparts;
    uint64_t total_bytes;
    uint64_t ntiles;
    uint64_t chunk_cap;
    uint64_t bm0_words;
    uint64_t bm1_words;
    uint64_t leaf_cap;
    uint32_t nonempty_parts;
    uint64_t max_part_bytes;
};

struct lthip_plan;
uint64_t lthip_plan_run_slots(const lthip_plan* plan); // slots of the plan's runs of leaf chaining values (lthip_part_run_base)
struct lthip_plan : PlanExtents
{
    int device;
    uint32_t min_chunk, avg_chunk, max_chunk;
    DivTest div;
    uint64_t capacity_bytes; // bytes the plan was created for (lthip_plan_resize_single may aim it at fewer)
    uint32_t cap_parts;      // parts / tiles the device tables were allocated for (lthip_plan_reaim)
    uint64_t cap_tiles;
    PartDev* d_parts;
    uint32_t* d_tile_part;
    // A plan of many parts and >= LTHIP_SLICE_MIN_BYTES also exists as LTHIP_SLICES plans over consecutive runs of its parts of
    // about equal bytes (lthip_chunk_hash: the candidate scans of the slices one after the other on one stream, the leaf hashing of
    // every slice behind its scan on a second stream -- the scan of slice i + 1 runs beside the hashing of slice i)
    lthip_plan* slice[8];
    uint32_t slice_first[9]; // slice i = parts [slice_first[i], slice_first[i + 1])
    uint32_t nslices;        // 0: the plan is run as one
    bool sliced;             // the slices are aimed at the plan's current parts
    bool walked;             // the plan's shape suits the walking scan (plan_walk_rule, decided at every aim; a slice has its own)
};
// The walking scan (k_buzhash_walk) hands whole parts to waves.  It needs more non-empty parts than the device holds K1 waves, so that
// the draw evens out what the parts cost, and no part so long that its wave works on alone at the end of the launch:
//   non-empty parts >= LTHIP_WALK_MIN_PARTS_PER_WAVE x resident waves
//   largest part x LTHIP_WALK_MAX_PART_DIV <= bytes / resident waves          (a part is at most that share of a wave's mean load)
// Where the thresholds lie was measured (profiles/walk_scan_sweep.txt: 64 GiB per step in two slices of 4096 resident
// waves each): 2 parts per wave (4 MiB files) still gain what 8 and 32 per wave gain, half a part per wave (16 MiB files) loses.
constexpr uint32_t LTHIP_WALK_MIN_PARTS_PER_WAVE = 2;
constexpr uint32_t LTHIP_WALK_MAX_PART_DIV = 2;
constexpr uint64_t LTHIP_SLICE_MIN_BYTES = 1ull << 30;
#ifndef LTHIP_SLICES
#define LTHIP_SLICES 2 /* plans that run the tile scan; a plan whose scan walks runs as one (plan_aim_slices; DESIGN.md §3, profiles/walk_regs_ab.txt) */
#endif

// ---------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------
enum ScratchSlot
{
    S_BM0 = 0,
    S_BM1,
    S_REGION,      // uint2 {rel_off, len} per bounded chunk slot
    S_PART_COUNT,  // u32 per part
    S_LEAF_COUNT,  // u32 per dense chunk (+1)
    S_LEAF_PREFIX, // u32 per dense chunk (+1)
    S_SCAN_TMP,
    S_CV,          // 8 x u32 per leaf
    S_LZ4_SEGS,    // segment descriptors
    S_LZ4_META,    // per-segment results
    S_LZ4_STREAM,  // per-segment sequence streams
    S_LZ4_BLOCKS,  // block tables
    S_TABLES,      // small H2D tables
    S_TABLES2,
    S_MISC,
    S_Z_LITS,  // zstd: literals per 4 KiB unit
    S_Z_RECS,  // zstd: sequence records per unit
    S_Z_ENC,   // zstd: encoded 128 KiB pieces
    S_Z_WORK,  // zstd: per-encoder-wave work area
    S_Z_SUB,   // zstd: content size of every unit's sub-block (u16 per 4 KiB unit) / decoder: sequence records
    S_LZ4_WORKLIST, // groups the stitch copy has to visit
    S_LZ4_CLASSIFY,  // two-pass match finder: list + flags of the groups with redundancy
    S_B3_WINDOWS,   // first range of every window of leaf slots (parents kernel)
    S_Z_FR,         // zstd decoder, frames of other encoders: per block {history in, start, history out}
    S_Z_ORG,        // ... and the origins (u32 per byte of output) of the payloads in flight
    S_Z_PERM,       // zstd decoder: the items in piece-major order, per-row counters, per-item done flags
    S_XCHG,         // multi-GPU exchange: range tables of lthip_exchange_reorder
    S_XCHG2,        // ... and the job tables of lthip_job_ordinals
    S_SLICE_OFFS,   // lthip_chunk_hash in slices: the chunk offsets / lengths / hashes / part tables of slices 1 .. S-1 before the join
    S_SLICE_LENS,
    S_SLICE_HASH,
    S_SLICE_FIRST,
    S_LEN_CLASS_ORDER, // BLAKE2s and Meow ranges: class histogram, cursors and the length-class order of the ranges
    S_WALK_TICKET,     // the walking scan's part counter
    S_RAW_BLOCKS,      // raw block images: per-block tables of lthip_raw_copy_blocks {payload offset, first chunk, chunk count}
    S_RAW_RUNS,        // ... its runs (one slot per chunk: source, destination, length), their piece counts and the scan of those
    S_RAW_TABLES,      // ... and the hash / BlockIndex tables of lthip_write_raw_block_images
    S_CARRY_RUNS,      // restore session, lthip_restore_carry: boundary flags and their scan, the runs, their piece counts and the scan of those
    S_ARCHIVE_ITEMS,   // archive writer, lthip_archive_writer_append: {source, destination, size} of the call's images
    S_CV_RUNS,         // 8 x u32 per leaf slot of the parts' runs (the walking scan that hashes)
    S_CV_SLOTS,        // ... and per dense chunk the slot of its first leaf in them (u32)
    S_COUNT
};

struct TimingRec
{
    int kid;
    hipEvent_t a, b;
};

struct lthip_ctx
{
    int device;
    hipStream_t stream;
    bool own_stream;
    lthip_ctx* slice_ctx;                // lazily created: context (private stream, scratch of its own) of lthip_chunk_hash's slices 1 .. S-1
    hipStream_t stream2;                 // lazily created side stream (non-blocking), see lthip_second_stream
    std::vector<hipEvent_t> sync_events; // ordering events between the two streams, reused round-robin
    size_t sync_next;
    char err[320];
    struct Stage // pinned staging slot of lthip_stage_upload
    {
        void* p;
        size_t cap;
        hipEvent_t done;
        bool used;
    };
    // two rings: uploads of up to LTHIP_STAGE_SMALL bytes (the per-batch tables of the codec phase: with one ring of 8 slots
    // lthip_ingest_write waited for the codec batch after batch) rotate through 64 slots of that size, larger ones (plans, the
    // tree's tables) through 8 slots that grow to what they have to hold
    Stage stage[8], stage_small[64];
    size_t stage_small_next;
    size_t stage_next;
    bool k5_lds_enabled[2][2]; // hipFuncAttributeMaxDynamicSharedMemorySize set on this context's device for k_lz4_segments<.., FMT, CLS> with units above 4 KiB
    bool k5h_lds_enabled[2]; // ... and for k_lz4_lanes2<FMT>
    void* scratch[S_COUNT];
    size_t scratch_cap[S_COUNT];
    bool timing;
    std::vector<TimingRec> pending;
    std::vector<hipEvent_t> free_events;
    const uint32_t* z_last_retry; // what the last lthip_zstd_decompress_blocks call of THIS context did (lthip_zstd_last_decode_stats)
    uint32_t z_last_payloads, z_last_foreign_blocks;
    double total_ms[LTHIP_K_COUNT];
    uint64_t launches[LTHIP_K_COUNT];
};

int lthip_fail(lthip_ctx* ctx, int code, const char* what, const char* detail);
// Runs a callable that returns an errno: std::bad_alloc becomes ENOMEM, "who: host tables" in the context's error text (no context: the code alone)
template <class F> int lthip_guarded(lthip_ctx* ctx, const char* who, F&& f)
{
    try
    {
        return f();
    }
    catch (const std::bad_alloc&)
    {
        return lthip_fail(ctx, ENOMEM, who, "host tables");
    }
}
// Waits for everything queued on the context's stream (the one place the library waits for a stream).  HOW a thread waits is the
// device's scheduling policy: lthip_set_blocking_waits (lthip_ctx.hip).
hipError_t lthip_stream_wait(lthip_ctx* ctx);

// Environment switches (ablations, debug paths) are read once per process and cached -- not per call: the plugins call from up to 256
// threads.  lthip_debug_reload_env() (tests: one process tries a path and its ablation) bumps the generation; a cache re-reads then.
extern volatile uint32_t g_lthip_env_gen;
struct LthipEnvInt
{
    // (function-local statics shared by every host thread of the plugin layer: the value is published before the generation it
    // belongs to, so a reader that sees the generation sees the value)
    const char* name;
    std::atomic<int> value{-1};     // atoi of the variable; -1 when it is not set
    std::atomic<uint32_t> seen{0};  // generation the value was read at (0: never)
    explicit LthipEnvInt(const char* n) : name(n) {}
    int get()
    {
        const uint32_t gen = g_lthip_env_gen;
        if (seen.load(std::memory_order_acquire) != gen)
        {
            const char* e = getenv(name);
            value.store(e ? atoi(e) : -1, std::memory_order_relaxed);
            seen.store(gen, std::memory_order_release);
        }
        return value.load(std::memory_order_relaxed);
    }
};
// The PRODUCT library reads eleven environment variables, all documented in README.md ("Environment"): LONGTAIL_HIP_DEVICE / _BATCH /
// _CODEC_BATCH / _LARGE_WINDOWS / _SMALL_WINDOWS (plugin layer), LTHIP_BATCH_BYTES, LTHIP_ORIGIN_MIB, LTHIP_COMM_TRANSPORT /
// _TIMEOUT_S / _SHM_SLOT / LTHIP_RCCL_PATH.  Every other LTHIP_* switch selects an earlier formulation of a kernel, a debug path or an experiment's
// parameter; those exist in the ABLATION build only (`make ablations`: -DLTHIP_ABLATIONS, build/ablations/liblongtail_hip.so, loaded
// by the differential tests and the A/B tools through LTHIP_LIB_PATH).  In the product build such a switch is a constant "not set",
// so the branches it guards fold away, and the kernels they launch are not compiled (#ifdef LTHIP_ABLATIONS around them).
#ifdef LTHIP_ABLATIONS
#define LTHIP_ABLATION_ENV(var, name) static LthipEnvInt var{name}
#else
struct LthipEnvOff
{
    constexpr int get() const { return -1; }
};
#define LTHIP_ABLATION_ENV(var, name) constexpr LthipEnvOff var{}
#endif
// Every device / pinned allocation of the library goes through these two.  Product build: hipMalloc / hipHostMalloc, nothing else.
// Ablation build: counted, and lthip_debug_fail_alloc(after, count) makes allocations after+1 .. after+count of the process fail with
// hipErrorOutOfMemory (tests/test_gpu_alloc_failures.py: ENOMEM out of CreateVersionIndex / WriteContent, nothing leaked, the same
// objects usable again -- the device-side counterpart of the reference's FailableStorageAPI tests, test/test.cpp:5677-5752).
#ifdef LTHIP_ABLATIONS
hipError_t lthip_hip_malloc(void** p, size_t bytes);
hipError_t lthip_hip_host_malloc(void** p, size_t bytes, unsigned flags);
#else
static inline hipError_t lthip_hip_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
static inline hipError_t lthip_hip_host_malloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
#endif
int lthip_scratch(lthip_ctx* ctx, int slot, size_t bytes, void** out);
lthip_ctx* lthip_store_ctx(const lthip_store* store); // the context a store belongs to (k_dedup.hip)
// A second in-order queue of the context for work that should overlap the main stream (callers order the two with
// events from lthip_sync_event and must make the main stream wait for the side stream before they return).
int lthip_second_stream(lthip_ctx* ctx, hipStream_t* out);
hipEvent_t lthip_sync_event(lthip_ctx* ctx);
// zstd frames of the "max" setting: 128 KiB pieces per chain (the match finder -- k_lz4.hip -- lets a piece see the one before it except
// in every LTHIP_ZSTD_CHAIN-th piece of a block; the decoder -- k_zstd.hip -- runs the pieces in between in order)
constexpr uint32_t LTHIP_ZSTD_CHAIN = 8;
uint64_t lthip_codec_batch_bytes(); // input bytes per internal codec batch (LTHIP_BATCH_BYTES, default 8 GiB)
uint64_t lthip_origin_budget_mib(); // (LTHIP_ORIGIN_MIB) arena of the restore paths' execution on origins (k_lz4.hip)
// Host table -> device without stalling the caller: the bytes are copied into one of a ring of pinned staging buffers and
// queued on `stream`; `h_src` may be freed on return, and the host does not wait for earlier work of the stream (a
// pageable hipMemcpyAsync + hipStreamSynchronize would wait for every kernel queued before it).
constexpr size_t LTHIP_STAGE_SMALL = 64u << 10;
int lthip_stage_upload(lthip_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, hipStream_t stream);

#define LTHIP_CHECK(ctx, expr)                                                          \
    do                                                                                  \
    {                                                                                   \
        hipError_t e__ = (expr);                                                        \
        if (e__ != hipSuccess)                                                          \
            return lthip_fail((ctx), e__ == hipErrorOutOfMemory ? ENOMEM : EIO, #expr, hipGetErrorString(e__)); \
    } while (0)

// More than 64 KiB of dynamic LDS has to be granted to a kernel explicitly, once per device.  `granted`: the call site's flags, one per
// device (plugin threads race here: the flags are atomic, and two threads that both set the attribute set the same value); a device
// outside the array is granted at every call.
inline int lthip_grant_lds(lthip_ctx* ctx, std::atomic<bool> (&granted)[64], std::initializer_list<const void*> kernels, size_t bytes)
{
    const bool known = ctx->device >= 0 && ctx->device < 64;
    if (known && granted[ctx->device].load(std::memory_order_acquire))
        return 0;
    for (const void* k : kernels)
        LTHIP_CHECK(ctx, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    if (known)
        granted[ctx->device].store(true, std::memory_order_release);
    return 0;
}

// timing brackets around a launch on ctx->stream
struct LaunchTimer
{
    lthip_ctx* ctx;
    TimingRec rec;
    bool on;
    hipStream_t stream;
    LaunchTimer(lthip_ctx* c, int kid, hipStream_t s = nullptr); // s == nullptr: the context's main stream
    ~LaunchTimer();
};

#define LTHIP_LAUNCH_CHECK(ctx)                                                          \
    do                                                                                   \
    {                                                                                    \
        hipError_t e__ = hipGetLastError();                                              \
        if (e__ != hipSuccess)                                                           \
            return lthip_fail((ctx), EIO, "kernel launch", hipGetErrorString(e__));      \
    } while (0)

// ---------------------------------------------------------------------------------------------------
// kernel launchers implemented in the k_*.hip files
// ---------------------------------------------------------------------------------------------------
int lthip_launch_tile_table(lthip_ctx* ctx, lthip_plan* plan);
int lthip_launch_buzhash(lthip_ctx* ctx, const lthip_plan* plan, const uint8_t* d_data, uint64_t* bm0, uint64_t* bm1);
// K1 + K2 in one launch, a wave per part (k_buzhash.hip: the walking scan); needs neither bitmap.  cv_runs != null: K3's leaf pass as
// well -- the wave that cuts a chunk hashes its leaves, chaining values to the part's run of cv_runs (8 words a slot, lthip_plan_run_slots
// of them, below 2^32) -- and lthip_launch_blake3_parents finishes the hashes behind compaction
int lthip_launch_buzhash_walk(lthip_ctx* ctx, const lthip_plan* plan, const uint8_t* d_data, uint2* region, uint32_t* part_count,
                              uint32_t* cv_runs);
uint32_t lthip_cu_count(int device);          // the device's compute units, asked for once per device
inline uint32_t lthip_k1_resident_waves(int device) { return 16u * lthip_cu_count(device); } // waves of a K1 launch that the device holds at a time: one 16-wave workgroup per CU
int lthip_launch_select(lthip_ctx* ctx, const lthip_plan* plan, const uint64_t* bm0, const uint64_t* bm1, uint2* region,
                        uint32_t* part_count);
// The payloads of raw (tag 0) block images (k_gather.hip): for each of `count` blocks the chunks [h_first[i], h_first[i] + h_count[i]) of the
// device lists, copied back to back from d_src + d_src_offsets[c] to d_arena + h_payload[i].  The chunk indices lie in
// [chunk_base, chunk_base + chunk_span); bytes_bound: an upper bound of the bytes copied (0 = unknown).  Host tables may be freed on
// return; nothing is waited for.
int lthip_raw_copy_blocks(lthip_ctx* ctx, uint32_t count, const uint32_t* h_first, const uint32_t* h_count, const uint64_t* h_payload,
                          uint32_t chunk_base, uint32_t chunk_span, const uint32_t* d_lens, const uint64_t* d_src_offsets, const void* d_src,
                          void* d_arena, uint64_t bytes_bound);
// The copy under it, for a caller that brings a run table of its own (the restore session's carry): run i = d_run_len[i] bytes from
// d_src + d_run_src[i] to d_dst + d_run_dst[i], any byte positions, cut into d_first_piece[i + 1] - d_first_piece[i] pieces
// (lthip_raw_pieces of the run's destination and length; 0 for a slot that holds no run; d_first_piece: slots + 1 entries, the
// exclusive scan of the piece counts).  pieces_bound: an upper bound of the pieces in all (0 = unknown).  Source and destination must not
// overlap.  Nothing is waited for.
int lthip_raw_copy_runs(lthip_ctx* ctx, const uint32_t* d_first_piece, uint32_t slots, const uint64_t* d_run_src, const uint64_t* d_run_dst,
                        const uint64_t* d_run_len, const void* d_src, void* d_dst, uint64_t pieces_bound);
constexpr uint32_t LTHIP_RAW_PIECE_VEC = 2048; // 16-byte vectors of a piece: 32 KiB, eight rounds of four requests per lane
__device__ __forceinline__ uint32_t lthip_raw_pieces(uint64_t dst, uint64_t len)
{
    if (len == 0)
        return 0u;
    uint64_t head = (16u - (dst & 15u)) & 15u;
    if (head > len)
        head = len;
    const uint64_t nvec = (len - head) >> 4;
    return nvec ? (uint32_t)((nvec + LTHIP_RAW_PIECE_VEC - 1) / LTHIP_RAW_PIECE_VEC) : 1u;
}
// The block writer of the ingest sessions (block_images.hip; the host side of a batch -- BlockBatch, Ranges -- and the tables the writer
// keeps -- BlockImageBufs -- are in ingest_buffers.h).  What a session says about the device side of a batch:
struct BlockBatchDev
{
    const void* places[3];         // the base pointers BlockBatch::place indexes, in the order the codec calls go
    uint32_t nplaces;
    const uint64_t* d_hashes;      // the chunk lists the batch's chunk ranges index ...
    const uint32_t* d_lens;
    uint32_t chunk_base;           // ... and the batch's first chunk in them
    const uint64_t* d_raw_offsets; // raw blocks: chunk c of the lists lies at d_raw_src + d_raw_offsets[c] (lthip_raw_copy_blocks)
    const void* d_raw_src;
    const uint64_t* d_bhash;       // the batch's entries of the block hashes and of the compressed sizes
    uint32_t* d_comp;
    void* d_arena;
};
struct BlockBatch;
struct BlockImageBufs;
struct Ranges;
// uploads the tables of `r` and copies its ranges from d_src to d_dst (lthip_gather_ranges)
int lthip_gather_upload(lthip_ctx* ctx, BlockImageBufs& w, const void* d_src, const Ranges& r, void* d_dst);
// the payloads of the batch's images: the raw copy, then the codec calls
int lthip_block_payloads(lthip_ctx* ctx, BlockImageBufs& w, BlockBatch& bt, const BlockBatchDev& dev);
// the bytes around them: the tables of k_stored_block_headers (with_tags: the blocks' tags too; without, every block carries
// cfg.compression_type), and its launch -- behind the launch that writes dev.d_bhash
int lthip_block_headers_upload(lthip_ctx* ctx, BlockImageBufs& w, const BlockBatch& bt, bool with_tags);
int lthip_block_headers(lthip_ctx* ctx, const BlockImageBufs& w, const BlockBatch& bt, const BlockBatchDev& dev, const lthip_ingest_config& cfg,
                        bool with_tags);
// k_stored_block_headers on the context's stream, for the bulk calls that bring tables of their own (kid: the timing class)
int lthip_launch_block_headers(lthip_ctx* ctx, int kid, const uint32_t* d_block_first_chunk, uint32_t nblocks, const uint64_t* d_chunk_hashes,
                               const uint32_t* d_chunk_lens, const uint64_t* d_block_hashes, uint32_t hash_identifier, uint32_t tag,
                               const uint32_t* d_block_tags, const uint32_t* d_raw_sizes, uint32_t* d_comp_sizes, const uint64_t* d_image_offsets,
                               void* d_arena, uint32_t raw_mode);
int lthip_launch_compact(lthip_ctx* ctx, const lthip_plan* plan, const uint2* region, const uint32_t* part_count,
                         uint32_t* d_part_first, uint64_t* d_chunk_offsets, uint32_t* d_chunk_lens);
int lthip_exclusive_scan_u32(lthip_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, uint64_t n_bound, const uint32_t* d_n,
                             int kid);
// BLAKE3-64 of count ranges (count = min(count_bound, *d_count) when d_count != null).  leaf_bound = upper bound on
// the total number of 1 KiB leaves (0 = unknown: read it back from the device), max_len = upper bound on a single
// range's length (0 = unknown).
int lthip_launch_blake3(lthip_ctx* ctx, const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_lens,
                        const uint32_t* d_count, uint64_t count_bound, uint64_t leaf_bound, uint64_t max_len,
                        uint64_t* d_hashes);

// The same for the chunks of a plan whose leaves the walking scan has hashed: the runs are moved to the dense leaf order, then the parents
struct lthip_b3_runs
{
    const uint32_t* d_cvs;        // the runs (lthip_part_run_base)
    const PartDev* d_parts;
    uint32_t nparts;              // > 0
    const uint32_t* d_part_first; // nparts + 1: the parts' first chunks in the dense lists (d_count = its last entry)
};
int lthip_launch_blake3_parents(lthip_ctx* ctx, const lthip_b3_runs& runs, const uint32_t* d_lens, const uint32_t* d_count,
                                uint64_t count_bound, uint64_t leaf_bound, uint64_t max_len, uint64_t* d_hashes);

int lthip_hash_ranges_known(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets, const uint32_t* d_lens,
                            uint32_t max_len, uint64_t leaf_total, uint64_t* d_hashes); // lthip_hash_ranges without its read-back

int lthip_launch_blake3_stream_batch(lthip_ctx* ctx, const void* d_data, uint32_t leaf0, uint32_t* d_stack, uint32_t depth_in, uint32_t merges);
int lthip_launch_blake3_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint32_t leaf0, const uint32_t* d_stack,
                                     uint32_t depth, uint64_t* d_out);
int lthip_launch_blake3_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out);

// A chain hash: one serial chain of compressions per message (BLAKE2s-64, k_blake2s.hip; Meow v0.5's low 64 bits, k_meow.hip).  The
// launches of a kind (k_hash_common.h: one policy over the kind's kernels); none of them reads anything back.
struct ChainHash
{
    // the digests of count ranges (count = min(count_bound, *d_count) when d_count != null)
    int (*ranges)(lthip_ctx* ctx, const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_lens, const uint32_t* d_count,
                  uint64_t count_bound, uint64_t* d_hashes);
    int (*one)(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out); // ONE input of at most 64 KiB, read where it lies
    int (*stream)(lthip_ctx* ctx, const void* d_data, uint32_t len, uint32_t* d_state, int first, int final, uint64_t* d_out);
    uint32_t stream_batch; // bytes of a stream batch (LTHIP_B2S_STREAM_BATCH / LTHIP_MEOW_STREAM_BATCH)
};
const ChainHash* lthip_chain_blake2s(); // k_blake2s.hip
const ChainHash* lthip_chain_meow();    // k_meow.hip
// The length-class order of ranges in blocks of 1 << unit_shift bytes, longest first (lthip_hash.hip, shared by the chain hashes):
// *order = count_bound slots, *n_long = device count of the leading ranges of class long_class and above.  S_LEN_CLASS_ORDER scratch.
int lthip_len_class_order(lthip_ctx* ctx, const uint32_t* d_lens, const uint32_t* d_count, uint64_t count_bound, uint32_t unit_shift,
                          uint32_t long_class, const uint32_t** order, const uint32_t** n_long);

// The hash of a longtail hash type over device ranges: what the index builders call for path hashes, asset content hashes and block
// hashes.  'blk2' (LTHIP_HASH_BLAKE2) runs BLAKE2s, 'meow' (LTHIP_HASH_MEOW) Meow; every other identifier runs BLAKE3, exactly the
// code path of lthip_hash_ranges / lthip_hash_ranges_known (leaf_total 0 = unknown).
constexpr uint32_t LTHIP_HASH_BLAKE3 = 0x626c6b33u; // 'blk3', lib/blake3/longtail_blake3.c
constexpr uint32_t LTHIP_HASH_BLAKE2 = 0x626c6b32u; // 'blk2', lib/blake2/longtail_blake2.c
constexpr uint32_t LTHIP_HASH_MEOW = 0x6d656f77u;   // 'meow', lib/meowhash/longtail_meowhash.c
const ChainHash* lthip_chain_hash(uint32_t hash_identifier); // the kind of 'blk2' and 'meow', null for every other identifier
int lthip_hash_ranges_by_id(lthip_ctx* ctx, uint32_t hash_identifier, const void* d_data, uint64_t range_count, const uint64_t* d_offsets,
                            const uint32_t* d_lens, uint32_t max_len, uint64_t leaf_total, uint64_t* d_hashes);

int lthip_launch_from_buffer(lthip_ctx* ctx, const uint8_t* d_data, uint32_t n, uint32_t min_chunk, const DivTest& dv,
                             uint64_t* d_out);

// zstd front end (k_lz4.hip): the LZ4 match finder run with sequence output.  Per 4 KiB unit u of the batch (units
// are numbered block after block, `unit_base[b]` first): literals at d_lits + u*4096, records at d_recs + u*1024,
// ZbUnitMeta at d_meta + u (zstd_block_core.h).
// quality: LTHIP_ZSTD_Q_* (the parse the zstd settings select)
int lthip_launch_lz_sequences(lthip_ctx* ctx, const void* d_src, uint32_t block_count, const uint64_t* src_offsets,
                              const uint32_t* src_sizes, void* d_dst, const uint64_t* dst_offsets, const uint32_t* dst_caps,
                              uint8_t** d_lits, uint64_t** d_recs, void** d_meta, uint32_t* unit_base, uint64_t* total_units, int quality);

// A restore session over occurrences that lie on the device (restore.hip): `count` whole chunks, chunk d_hash[i] of d_len[i] bytes to
// byte d_dst[i] of the output.  The session behaves as one lthip_restore_create made, with no asset selected; the list is copied on the
// context's stream and may be freed once that has run.  who: the name refusals carry.
struct lthip_occurrence_list
{
    uint32_t hash_identifier;
    uint64_t count;
    const uint64_t* d_hash;
    const uint32_t* d_len;
    const uint64_t* d_dst;
};
int lthip_restore_create_occurrences(lthip_ctx* ctx, const lthip_restore_config* cfg, const lthip_occurrence_list* list, const void* store_index,
                                     size_t si_size, uint64_t out_bytes, const char* who, lthip_restore** out);
uint64_t lthip_restore_outstanding(const lthip_restore* r); // needed blocks that were not delivered yet

static inline uint64_t div_up_u64(uint64_t a, uint64_t b) { return (a + b - 1) / b; }
