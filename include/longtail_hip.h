/* longtail_hip.h -- C ABI of liblongtail_hip.so: MI355X (gfx950) implementations of longtail's
 * chunk -> hash -> compress hot path.
 *
 * Two layers, both plain C (pointers + sizes, errno-style int results, no C++/torch types):
 *
 *  A. PLUGIN CONSTRUCTORS -- what a longtail embedder binds instead of the CPU constructors.  They
 *     return longtail's own struct-of-function-pointer objects (include/longtail_abi.h), so they drop
 *     into Longtail_CreateVersionIndex / Longtail_WriteContent / the registries unchanged.
 *
 *  B. BULK DEVICE API (lthip_*) -- the thin shim over the HIP kernels that layer A is written on, for
 *     callers that already hold asset bytes in HBM (bench.py, the multi-GPU driver, tests).
 *
 * Every entry point cites the reference interface it replaces.
 */
#ifndef LONGTAIL_HIP_H
#define LONGTAIL_HIP_H

#include "longtail_abi.h"

#if defined(_WIN32)
#define LTHIP_EXPORT
#else
#define LTHIP_EXPORT __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* =====================================================================================================
 * A. plugin constructors
 * =================================================================================================== */

/* Replaces Longtail_CreateHPCDCChunkerAPI() (lib/hpcdcchunker/longtail_hpcdcchunker.h:10,
 * implementation longtail_hpcdcchunker.c:332-589).  GetMinChunkSize -> 48.  NextChunk drains the
 * feeder into pinned host memory (windows of up to 64 MiB), computes ALL cut points and ALL chunk
 * hashes of the window on the GPU, then hands out ranges whose `buf` points into the pinned window;
 * ESPIPE + {0,total,0} at end of stream exactly like the reference. */
LTHIP_EXPORT struct Longtail_ChunkerAPI* Longtail_CreateHipChunkerAPI(void);

/* Replaces Longtail_CreateBlake3HashAPI() (lib/blake3/longtail_blake3.h, implementation
 * longtail_blake3.c:6-141).  GetIdentifier -> 0x626c6b33 ('blk3') so indexes are interchangeable with
 * CPU-built ones.  HashBuffer on a range previously handed out by a HIP chunker returns the digest the
 * GPU already computed; any other buffer is hashed on the GPU on demand. */
LTHIP_EXPORT struct Longtail_HashAPI* Longtail_CreateHipBlake3HashAPI(void);

/* Replaces Longtail_CreateBlake2HashAPI() (lib/blake2/longtail_blake2.h, implementation longtail_blake2.c).  GetIdentifier ->
 * 0x626c6b32 ('blk2'); digests are unkeyed BLAKE2s with an 8-byte output read as a little-endian u64 (blake2s(out, 8, data, len,
 * 0, 0), longtail_blake2.c).  HashBuffer, BeginContext / Hash / EndContext behave as the BLAKE3 object's: O(1) host state per
 * context, EndContext failures latched for Longtail_Hip_GetLastError.  Paired with a HIP chunker: the window's chunks get a BLAKE2
 * digest table, filled by the first HashBuffer of one of them (one lthip_blake2s_ranges over the whole window, from the window's
 * device copy or uploaded again from the pinned window); later HashBuffer calls of the window read it.  Other buffers are hashed on
 * the GPU one by one (lthip_blake2s_one up to 64 KiB).  The chunker itself still computes BLAKE3 digests, unused here. */
LTHIP_EXPORT struct Longtail_HashAPI* Longtail_CreateHipBlake2HashAPI(void);

/* Replaces Longtail_CreateMeowHashAPI() (lib/meowhash/longtail_meowhash.h, implementation longtail_meowhash.c).  GetIdentifier ->
 * 0x6d656f77 ('meow'); digests are the low 64 bits of Meow hash v0.5 with the default seed (MeowBegin / MeowAbsorb / MeowEnd,
 * longtail_meowhash.c).  The entry points behave as the BLAKE2 object's, window digest table included: a chunker window filled by one
 * object is filled again for the other, and each gets its own digests. */
LTHIP_EXPORT struct Longtail_HashAPI* Longtail_CreateHipMeowHashAPI(void);

/* WHEN TO CONSTRUCT THE CODEC OBJECTS.  One stored block per Compress call crosses the link twice: the HIP codec objects pay on data that
 * compresses -- WriteContent at 32 bikeshed workers: LZ4 31-47 GB/s against the reference codec's 22-25, ZStd 33-35 against 7-14 -- and
 * lose on incompressible bytes, where the CPU's LZ4 is a memcpy (25-29 against 56-105 GB/s): there bind the reference's own LZ4 beside
 * the HIP chunker + hash, or use the bulk session (lthip_ingest_*), which never brings payload bytes back through Compress
 * (INTEGRATION.md "Which codec object to bind"; numbers: the bench line's secondary.*.drop_in, profiles/r06q_*).
 *
 * Replaces Longtail_CreateLZ4CompressionAPI() / Longtail_CompressionRegistry_CreateForLZ4()
 * (lib/lz4/longtail_lz4.h:10-12, longtail_lz4.c:12-23,47-123).  Same type id 'lz42', same bound
 * (n + n/255 + 16), payload = one LZ4 *block* that LZ4_decompress_safe decodes. */
LTHIP_EXPORT struct Longtail_CompressionAPI* Longtail_CreateHipLZ4CompressionAPI(void);
LTHIP_EXPORT struct Longtail_CompressionAPI* Longtail_CompressionRegistry_CreateForHipLZ4(uint32_t compression_type, uint32_t* out_settings);
LTHIP_EXPORT uint32_t Longtail_GetHipLZ4DefaultQuality(void);

/* Replaces Longtail_CreateZStdCompressionAPI() / Longtail_CompressionRegistry_CreateForZstd()
 * (lib/zstd/longtail_zstd.h:10-16, longtail_zstd.c:30-41,72-177).  Type ids 'ztd1'..'ztd5'; the setting selects one of three
 * parses (lthip_zstd_quality_of_settings: 'ztd1' / 'ztd2' default, 'ztd4' high, 'ztd3' / 'ztd5' max; unknown ids -> default, exactly
 * like longtail_zstd.c:43-60).  Compress: one zstd frame per block -- RLE / Compressed (LZ sequences, Huffman literals, FSE sequences) / Raw
 * blocks -- that ZSTD_decompressDCtx decodes.  Decompress: any zstd frame(s) without a dictionary, e.g. the reference
 * encoder's; malformed input -> EINVAL (longtail_zstd.c:168-172). */
LTHIP_EXPORT struct Longtail_CompressionAPI* Longtail_CreateHipZStdCompressionAPI(void);
LTHIP_EXPORT struct Longtail_CompressionAPI* Longtail_CompressionRegistry_CreateForHipZstd(uint32_t compression_type, uint32_t* out_settings);

/* Route the plugins' host allocations through the embedder's allocator, e.g. Longtail_Alloc /
 * Longtail_Free (src/longtail.h:967-974) so memtracer leak checks see them.  Default malloc/free. */
typedef void* (*Longtail_Hip_AllocFunc)(const char* context, size_t size);
typedef void (*Longtail_Hip_FreeFunc)(void* p);
LTHIP_EXPORT void Longtail_Hip_SetAllocator(Longtail_Hip_AllocFunc alloc_func, Longtail_Hip_FreeFunc free_func);

/* GPU used by plugin objects created afterwards (default: $LONGTAIL_HIP_DEVICE or 0). */
LTHIP_EXPORT int Longtail_Hip_SetDevice(int device);
/* OPTIONAL, and if used the embedder's FIRST call into this library, before the process has touched the GPU: host threads waiting
 * for the device SLEEP until the interrupt (hipSetDeviceFlags(hipDeviceScheduleBlockingSync) on the plugin device) instead of polling.
 * The job system calls the blocking Longtail_*API functions from 32-256 threads at once; polling was a third of the drop-in path's
 * CPU time, and under a container's CPU quota that is throughput: CreateVersionIndex through the plugins 30 -> 40 GB/s at 32 workers,
 * UpSync 13.9 -> 16.5 (profiles/r06_dropin_scaling.txt; bench.py's drop_in legs run in a process of their own that makes this call).
 * It is the device's policy, PROCESS-WIDE, and must not be switched in a process that already ran GPU work: waits on completion signals
 * made before the switch may never return (observed).  Returns 0 or an errno; the library never makes this call on its own. */
LTHIP_EXPORT int Longtail_Hip_SetBlockingWaits(int on);
LTHIP_EXPORT int lthip_set_blocking_waits(int device, int on); /* the call behind it */

/* HashAPI.Hash / EndContext return no error code (longtail_blake3.c:43-79 cannot fail; a GPU path can: allocation, copy, no
 * device).  The first errno of such a call on the calling thread is latched; this returns and clears it (0 = none). */
LTHIP_EXPORT int Longtail_Hip_GetLastError(void);

/* Pinned host memory currently held by the chunker windows.  Windows are pooled in two classes -- 2 MiB (at most
 * $LONGTAIL_HIP_SMALL_WINDOWS, default 256) and 64 MiB (at most $LONGTAIL_HIP_LARGE_WINDOWS, default 32) -- so the bound is
 * about 0.5 + 2 GiB (and as much HBM) however many chunkers longtail's job system keeps alive; a thread that needs a window beyond
 * the cap waits for one to be released.  The reference pools 4 * max_chunk bytes per chunker (hpcdcchunker.c:148-171). */
LTHIP_EXPORT uint64_t Longtail_Hip_PinnedBytes(void);
/* Diagnostics of the small-window batcher (plugin_batch.c): GPU submissions made and windows carried by them since the library
 * was loaded; windows / batches = how many chunkers shared a submission on average. */
LTHIP_EXPORT void Longtail_Hip_BatchStats(uint64_t* out_batches, uint64_t* out_windows);
/* ... and of the codec objects: submissions of the dispatcher that runs concurrent Compress / Decompress calls together, blocks in them */
LTHIP_EXPORT void Longtail_Hip_CodecBatchStats(uint64_t* out_submissions, uint64_t* out_blocks);
/* ... and of its content-hash memo: digest arrays remembered, HashBuffer calls answered from them */
LTHIP_EXPORT void Longtail_Hip_MemoStats(uint64_t* out_puts, uint64_t* out_hits);

/* =====================================================================================================
 * B. bulk device API
 * =================================================================================================== */

typedef struct lthip_ctx lthip_ctx;   /* one GPU + one stream + scratch pools; NOT thread-safe: one per host thread */
typedef struct lthip_plan lthip_plan; /* device-resident description of a batch of parts */

/* hip_stream: the hipStream_t to launch on, e.g. torch.cuda.current_stream().cuda_stream; NULL is HIP's default
 * (null) stream, exactly as in every HIP API; LTHIP_STREAM_PRIVATE asks for a private non-blocking stream owned
 * by the context (what the plugin layer uses: one per host thread). */
#define LTHIP_STREAM_PRIVATE ((void*)(intptr_t)-1)
LTHIP_EXPORT int lthip_ctx_create(int device, void* hip_stream, lthip_ctx** out_ctx);
LTHIP_EXPORT void lthip_ctx_destroy(lthip_ctx* ctx);
LTHIP_EXPORT int lthip_ctx_sync(lthip_ctx* ctx);
LTHIP_EXPORT const char* lthip_ctx_error(const lthip_ctx* ctx); /* text of the last failure */
LTHIP_EXPORT int lthip_device_count(void);
/* Identity of the sources the library was built from: the first 16 hex digits of the sha256 tools/build_id.py computes over
 * longtail_amd/csrc/ and include/.  A test recomputes it from the tree, so a stale binary cannot pass for HEAD. */
LTHIP_EXPORT const char* lthip_build_id(void);
/* Version of the BINARY interface of section B: bumped whenever a struct of this header grows or changes layout, an enum value
 * moves, or an entry point changes its signature (new entry points alone do not bump it).  An embedder built against this header
 * checks  lthip_abi_version() == LTHIP_ABI_VERSION  once after loading the library.
 *   1  rounds 1-3      2  round 4: lthip_ingest_result.gathered_bytes appended, LTHIP_K_COUNT 9 -> 10
 *   3  round 5: lthip_ingest_result starts with struct_size (set by the caller; the library writes no more than that)
 *   4  lthip_store and the sessions' set_store / store_stats: a session with a store attached writes what the store lacks, so
 *      unique_local of the stream session's result may be below unique_all
 *      (still 4 with LTHIP_CODEC_BY_TAG, lthip_block_index_size and lthip_write_raw_block_images: a new enum VALUE behind the existing
 *      ones and new entry points -- no struct changes, no value moves, no signature changes) */
#define LTHIP_ABI_VERSION 4
LTHIP_EXPORT int lthip_abi_version(void);

/* Memory helpers so that plain-C callers (the plugin layer) need no HIP headers.  Copies are
 * asynchronous on the context's stream: lthip_ctx_sync() before reading a d2h destination. */
LTHIP_EXPORT int lthip_malloc_device(lthip_ctx* ctx, size_t bytes, void** out);
LTHIP_EXPORT void lthip_free_device(lthip_ctx* ctx, void* p);
LTHIP_EXPORT int lthip_malloc_pinned(lthip_ctx* ctx, size_t bytes, void** out);
LTHIP_EXPORT void lthip_free_pinned(lthip_ctx* ctx, void* p);
LTHIP_EXPORT int lthip_copy_h2d(lthip_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
LTHIP_EXPORT int lthip_copy_d2h(lthip_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
/* The same copy made by the compute units instead of the copy engines, either direction, `dst` and `src` 16-byte aligned, the
 * host side PINNED (lthip_malloc_pinned / hipHostMalloc).  On the MI355X boxes measured (profiles/r05_pcie_duplex.json) the copy
 * engines serve one direction at a time -- h2d and d2h queued on two streams take the sum of their times -- while kernel copies
 * in both directions overlap (46 GB/s each against 57 GB/s alone): a loop that streams slices in and block images out uses this
 * (and lthip_gather_ranges, which accepts pinned host memory as source or destination too) on contexts of their own. */
LTHIP_EXPORT int lthip_link_copy(lthip_ctx* ctx, void* dst, const void* src, size_t bytes);

/* Per-kernel timing with HIP events on the context's stream (bench.py roofline leg). */
enum lthip_kernel_id
{
    LTHIP_K_BUZHASH = 0,  /* candidate scan                     (hpcdcchunker.c:266-306) */
    LTHIP_K_SELECT = 1,   /* cut selection                      (hpcdcchunker.c:250-264,281-309) */
    LTHIP_K_COMPACT = 2,  /* scans + compaction of chunk lists  (src/longtail.c:2499-2517) */
    LTHIP_K_B3_LEAF = 3,  /* BLAKE3 leaves                      (blake3.c:118-151) */
    LTHIP_K_B3_PARENT = 4,/* BLAKE3 parents + root              (blake3.c:216-249,576-618) */
    LTHIP_K_LZ4_SEG = 5,  /* LZ4 segment encoder                (lz4.c:930-1338) */
    LTHIP_K_LZ4_STITCH = 6,/* LZ4 stitch scan + compaction copy */
    LTHIP_K_OTHER = 7,
    LTHIP_K_ZSTD_ENC = 8, /* zstd entropy stage (Huffman literals, FSE sequences), one wave per 128 KiB piece */
    LTHIP_K_GATHER = 9,   /* device block assembly: chunk ranges -> contiguous block images (src/longtail.c:4640-4721) */
    LTHIP_K_BLAKE2S = 10, /* BLAKE2s-64 ('blk2'): ranges, one input, streaming (lib/blake2/longtail_blake2.c) */
    LTHIP_K_COUNT = 11
};
LTHIP_EXPORT int lthip_timing_enable(lthip_ctx* ctx, int on);
LTHIP_EXPORT int lthip_timing_reset(lthip_ctx* ctx);
/* resolves pending events (synchronises the stream); total milliseconds and launch count per kernel id */
LTHIP_EXPORT int lthip_timing_get(lthip_ctx* ctx, int kernel_id, double* out_total_ms, uint64_t* out_launches);

/* ---- phase 1: chunk + hash ------------------------------------------------------------------------
 * A *part* is what the reference chunks with one chunker: one (asset, target_chunk_size*1024-byte
 * segment) job of ChunkAssets (src/longtail.c:2396-2458).  Parts live in one device buffer at
 * 16-byte aligned offsets.  min/avg/max as computed by src/longtail.c:1985-1987. */
LTHIP_EXPORT int lthip_plan_create(lthip_ctx* ctx, uint32_t part_count, const uint64_t* part_offsets /*host*/,
                                   const uint64_t* part_sizes /*host*/, uint32_t min_chunk, uint32_t avg_chunk,
                                   uint32_t max_chunk, lthip_plan** out_plan);
/* A plan of ONE part (created with part_count 1, offset 0, size = capacity) aimed at `size` <= capacity bytes: no allocation, no
 * kernel, no synchronisation -- the plugin chunker keeps one plan per window and re-aims it at every refill. */
LTHIP_EXPORT int lthip_plan_resize_single(lthip_ctx* ctx, lthip_plan* plan, uint64_t size);
/* The plan aimed at ANOTHER set of parts: at most as many as it was created with, and no more 16 KiB tiles in total; no
 * allocation, no synchronisation (the tables are rewritten on the context's stream).  The plugin layer's batcher keeps one plan of
 * N window slots and aims it at the windows of every submission. */
LTHIP_EXPORT int lthip_plan_reaim(lthip_ctx* ctx, lthip_plan* plan, uint32_t part_count, const uint64_t* part_offsets /*host*/,
                                  const uint64_t* part_sizes /*host*/);
/* ctx may be NULL (e.g. the creating thread's context is gone): the device is synchronised instead of the stream */
LTHIP_EXPORT void lthip_plan_destroy(lthip_ctx* ctx, lthip_plan* plan);
/* upper bound on the number of chunks the plan can produce (size the output arrays with it) */
LTHIP_EXPORT uint64_t lthip_plan_chunk_capacity(const lthip_plan* plan);
/* The number of slices the next lthip_chunk_hash with hashes runs this plan in, 1 .. 8: plans of >= 1 GiB in >= 2 parts run as slices
 * on two streams (the candidate scan of slice k + 1 beside the leaf hashing of slice k; results identical to the single pass): 2 for
 * plans that run the tile scan, 1 for plans whose scan walks; LTHIP_SLICES in the ablation build; 1 = the single pass.  Per-kernel timings (lthip_timing_get) of the scan and
 * the leaf hashing of a sliced call OVERLAP: their sum exceeds the wall time of the call. */
LTHIP_EXPORT uint32_t lthip_plan_slices(const lthip_plan* plan);
/* How many of those lthip_plan_slices scans are WALKING scans: a plan (or slice) of many more non-empty parts than the device holds
 * scan waves, none of them long against a wave's share of the bytes, is scanned by waves that own whole parts and walk them chunk by
 * chunk, skipping the bytes below every chunk's minimum length (candidate scan and cut selection in one launch, timed as
 * LTHIP_K_BUZHASH; no LTHIP_K_SELECT launch).  Decided from the plan's shape at every aim; every other plan runs the tile scan.  The
 * results are the same, bit for bit. */
LTHIP_EXPORT uint32_t lthip_plan_walked_scans(const lthip_plan* plan);

/* Runs buzhash scan -> cut selection -> compaction -> (if d_chunk_hashes) BLAKE3 on the stream.
 * Outputs (device pointers, capacity >= lthip_plan_chunk_capacity):
 *   d_chunk_offsets[i]  byte offset of chunk i in d_data            (dense, parts in order)
 *   d_chunk_lens[i]     its length
 *   d_chunk_hashes[i]   first 8 BLAKE3 bytes as LE u64              (may be NULL: chunk only)
 *   d_part_first[p]     index of the first chunk of part p, d_part_first[part_count] = total
 * Asynchronous; *out_total (host, may be NULL) is filled after an internal stream sync when given. */
LTHIP_EXPORT int lthip_chunk_hash(lthip_ctx* ctx, const lthip_plan* plan, const void* d_data, uint64_t* d_chunk_offsets,
                                  uint32_t* d_chunk_lens, uint64_t* d_chunk_hashes, uint32_t* d_part_first,
                                  uint64_t* out_total);

/* HPCDCChunker_NextChunkFromBuffer (hpcdcchunker.c:452-523) on a device buffer of `size` > min_chunk bytes:
 * *out_len = length of the chunk at its front.  Reproduces the reference's window-seeding quirk (the rolling
 * window starts from buf[0..48) instead of buf[min-48..min), :488-494), which NextChunk does not have.
 * Synchronous (one small kernel + read-back). */
LTHIP_EXPORT int lthip_chunk_from_buffer(lthip_ctx* ctx, const void* d_data, uint64_t size, uint32_t min_chunk,
                                         uint32_t avg_chunk, uint32_t max_chunk, uint64_t* out_len);

/* Host-side evaluation of the division-free cut test the kernels use (1 when h % d == d-1 for the discriminator
 * d): exported so the arithmetic can be checked exhaustively without a GPU. */
LTHIP_EXPORT int lthip_divtest_eval(uint32_t discriminator, uint32_t hash);

/* BLAKE3-64 of arbitrary device ranges: d_hashes[i] = blake3(d_data + d_offsets[i], d_lens[i]).
 * Same contract as Blake3Hash_HashBuffer (longtail_blake3.c:81-102); len 0 is legal. */
LTHIP_EXPORT int lthip_hash_ranges(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets,
                                   const uint32_t* d_lens, uint32_t max_len /*upper bound of d_lens[], 0 = unknown*/,
                                   uint64_t* d_hashes);

/* BLAKE3-64 of ONE input of at most 64 KiB in one launch, read where it lies and answered where `out` points: both must be device
 * accessible (pinned host memory from lthip_malloc_pinned, or device memory); `in` may have any alignment.  What the plugin layer's
 * HashBuffer uses for path strings and hash arrays.  Asynchronous on the context's stream; EINVAL above 64 KiB. */
LTHIP_EXPORT int lthip_hash_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out);

/* Streaming BLAKE3-64 with O(1) state (Blake3Hash_BeginContext/_Hash/_EndContext, longtail_blake3.c:24-79): the caller cuts the
 * stream into batches of LTHIP_B3_STREAM_BATCH bytes (device memory, 16-byte aligned), calls lthip_b3_stream_batch for the batches
 * in order -- a batch only when at least one byte follows it -- and lthip_b3_stream_final with the rest (1 .. one batch of bytes, or
 * 0 bytes after 0 batches: the empty stream).  d_stack: LTHIP_B3_STREAM_STACK_BYTES of device memory per stream; d_out: device or
 * pinned host memory.  Asynchronous on the context's stream.  Streams below 4 TiB. */
#define LTHIP_B3_STREAM_BATCH (1u << 20)
#define LTHIP_B3_STREAM_STACK_BYTES 2048u
LTHIP_EXPORT int lthip_b3_stream_batch(lthip_ctx* ctx, const void* d_data, uint64_t batch_index, void* d_stack);
LTHIP_EXPORT int lthip_b3_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, const void* d_stack,
                                       uint64_t* d_out);

/* BLAKE3-64 of runs of 64-bit values: d_out[i] = blake3(bytes of d_values[d_first[i] .. d_first[i+1])), i < run_count.  Over the
 * chunk hashes and the part table of lthip_chunk_hash: every part's content hash (src/longtail.c:2518-2537 for a one-part asset). */
/* ..._bounded: the caller knows upper bounds of d_first[run_count] - d_first[0] (all values) and of the longest run: with runs of at
 * most 32768 values the call then never waits for the device (no read-back of the counts).  0 = unknown. */
LTHIP_EXPORT int lthip_hash_runs_u64_bounded(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                             uint64_t total_values_bound, uint64_t run_values_bound, uint64_t* d_out);
LTHIP_EXPORT int lthip_hash_runs_u64(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                     uint64_t* d_out);

/* ---- BLAKE2s-64, the 'blk2' hash type (k_blake2s.hip) ----------------------------------------------------------------------
 * Digest = the first 8 bytes of unkeyed BLAKE2s with outlen 8, as a little-endian u64 (longtail_blake2.c: blake2s(out, 8, data, len,
 * 0, 0)); == int.from_bytes(hashlib.blake2s(data, digest_size=8).digest(), "little").  Same contracts as the BLAKE3 entry points above.
 * lthip_blake2s_ranges: d_hashes[i] = blake2s(d_data + d_offsets[i], d_lens[i]); len 0 is legal, ranges may overlap and start at any
 * byte.  max_len is accepted for symmetry with lthip_hash_ranges and may be 0.  Never waits for the device.
 * lthip_blake2s_ranges_dev: the number of ranges is min(count_bound, *d_count) with d_count on the device -- e.g. d_part_first +
 * part_count of lthip_chunk_hash(..., d_chunk_hashes = NULL, ...) with count_bound = lthip_plan_chunk_capacity: BLAKE2 chunk hashes
 * queued behind the chunker without a host synchronisation. */
LTHIP_EXPORT int lthip_blake2s_ranges(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets,
                                      const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes);
LTHIP_EXPORT int lthip_blake2s_ranges_dev(lthip_ctx* ctx, const void* d_data, uint64_t count_bound, const uint32_t* d_count,
                                          const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes);
/* ONE input of at most 64 KiB read where it lies, as lthip_hash_one (pinned host or device memory for `in` and `out`, any alignment);
 * EINVAL above 64 KiB.  Asynchronous on the context's stream. */
LTHIP_EXPORT int lthip_blake2s_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out);
/* BLAKE2s-64 of runs of 64-bit values, the contracts of lthip_hash_runs_u64[_bounded] (the bounds only spare the BLAKE3 call its read-back;
 * the BLAKE2s call never reads back and ignores them). */
LTHIP_EXPORT int lthip_blake2s_runs_u64_bounded(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                                uint64_t total_values_bound, uint64_t run_values_bound, uint64_t* d_out);
LTHIP_EXPORT int lthip_blake2s_runs_u64(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                        uint64_t* d_out);
/* Streaming BLAKE2s-64 with O(1) state (Blake2Hash_BeginContext/_Hash/_EndContext).  The state is LTHIP_B2S_STREAM_STATE_BYTES of
 * device memory ({h[8], bytes so far}; no initialisation needed).  The caller cuts the stream into batches of LTHIP_B2S_STREAM_BATCH
 * bytes (device memory, 16-byte aligned) and calls lthip_b2s_stream_batch for them in order -- a batch only when at least one byte
 * follows it, because BLAKE2 marks the LAST block of the stream -- then lthip_b2s_stream_final with the rest (1 .. one batch of bytes,
 * or 0 bytes after 0 batches: the empty stream).  d_out: device or pinned host memory.  Asynchronous on the context's stream.  One
 * stream is one serial chain of 64-byte compressions on one quad of lanes: a batch costs its 16 384 compressions back to back. */
#define LTHIP_B2S_STREAM_BATCH (1u << 20)
#define LTHIP_B2S_STREAM_STATE_BYTES 64u
LTHIP_EXPORT int lthip_b2s_stream_batch(lthip_ctx* ctx, const void* d_data, uint64_t batch_index, void* d_state);
LTHIP_EXPORT int lthip_b2s_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, void* d_state,
                                        uint64_t* d_out);

/* ---- Meow hash v0.5, 64 bits: the 'meow' hash type (k_meow.hip) --------------------------------------------------------------
 * Digest = the low 64 bits of MeowEnd after MeowBegin(MeowDefaultSeed) and MeowAbsorb of the bytes (longtail_meowhash.c:43-50).  The
 * entry points have the contracts of the BLAKE2s ones above, name for name: _ranges[_dev], _one (at most 64 KiB, any alignment),
 * _runs_u64[_bounded] (the bounds are ignored), and the stream pair.  Meow's absorb step takes whole 256-byte blocks, and a batch is
 * 4096 of them; as for BLAKE2s, a batch is sent only when at least one byte follows it, and the final call takes the rest (1 .. one
 * batch of bytes, or 0 bytes after 0 batches).  The state is {eight 128-bit registers, bytes so far}.  A stream is one serial chain on
 * one quad of lanes. */
#define LTHIP_MEOW_STREAM_BATCH LTHIP_B3_STREAM_BATCH
#define LTHIP_MEOW_STREAM_STATE_BYTES 136u
LTHIP_EXPORT int lthip_meow_ranges(lthip_ctx* ctx, const void* d_data, uint64_t range_count, const uint64_t* d_offsets,
                                   const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes);
LTHIP_EXPORT int lthip_meow_ranges_dev(lthip_ctx* ctx, const void* d_data, uint64_t count_bound, const uint32_t* d_count,
                                       const uint64_t* d_offsets, const uint32_t* d_lens, uint32_t max_len, uint64_t* d_hashes);
LTHIP_EXPORT int lthip_meow_one(lthip_ctx* ctx, const void* in, uint32_t len, uint64_t* out);
LTHIP_EXPORT int lthip_meow_runs_u64_bounded(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                             uint64_t total_values_bound, uint64_t run_values_bound, uint64_t* d_out);
LTHIP_EXPORT int lthip_meow_runs_u64(lthip_ctx* ctx, const uint64_t* d_values, const uint32_t* d_first, uint32_t run_count,
                                     uint64_t* d_out);
LTHIP_EXPORT int lthip_meow_stream_batch(lthip_ctx* ctx, const void* d_data, uint64_t batch_index, void* d_state);
LTHIP_EXPORT int lthip_meow_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, void* d_state,
                                         uint64_t* d_out);

/* ---- phase 2: per-block compression ----------------------------------------------------------------
 * One call compresses a batch of stored blocks (the unit of CompressBlock, compressblockstore.c:67-141).
 * Block b = d_src[src_offsets[b] .. +src_sizes[b]) -> d_dst[dst_offsets[b] ..) with capacity dst_caps[b];
 * d_out_sizes[b] = payload size, or 0 when it does not fit (LZ4CompressionAPI_Compress -> ENOMEM).
 * The offset/size tables are HOST arrays (copied to the device by the call).  The calls queue their work on the context's
 * stream and return (results are ready after lthip_ctx_sync or any later work on the stream); a call of any size is cut
 * into internal batches of LTHIP_BATCH_BYTES of input (environment, default 8 GiB) so that the scratch stays bounded.
 *
 * Windows -- for the four block codec calls (lthip_lz4_compress_blocks, lthip_lz4_decompress_blocks,
 * lthip_zstd_compress_blocks[_q], lthip_zstd_decompress_blocks):
 *   - A call writes no byte of d_dst outside [dst_offsets[b], dst_offsets[b] + dst_caps[b]) for any block b, whatever the payload
 *     contains and whether the block's result is a size, 0 or 0xFFFFFFFF.
 *   - Bytes inside the window beyond the returned size are unspecified, and so is the whole window of a refused block (result 0 from
 *     an encoder, 0xFFFFFFFF from a decoder): the encoders place bytes before they know whether the payload fits, a decoder stops
 *     where it finds the damage.
 *   - Source and destination windows may lie at any byte position, and the destination windows of different blocks may touch, with
 *     no gap between them.
 *   - Reads stay inside the 16-byte aligned hull of a block's source window (k_lz4_decode.hip, k_copy.h): a source needs no padding
 *     beyond the allocation granule of the device.
 * tests/test_gpu_codec_windows.py holds the calls to the first three (tests/codec_windows_util.py: guarded and packed layouts). */
LTHIP_EXPORT size_t lthip_lz4_bound(size_t size); /* LZ4_COMPRESSBOUND, lib/lz4/ext/lz4.h:215 */
LTHIP_EXPORT int lthip_lz4_compress_blocks(lthip_ctx* ctx, const void* d_src, uint32_t block_count,
                                           const uint64_t* src_offsets, const uint32_t* src_sizes, void* d_dst,
                                           const uint64_t* dst_offsets, const uint32_t* dst_caps,
                                           uint32_t* d_out_sizes, int segment_log2 /*0 = default*/);
/* LZ4_decompress_safe semantics per block; d_out_sizes[b] = decoded size or 0xFFFFFFFF on malformed input */
LTHIP_EXPORT int lthip_lz4_decompress_blocks(lthip_ctx* ctx, const void* d_src, uint32_t block_count,
                                             const uint64_t* src_offsets, const uint32_t* src_sizes, void* d_dst,
                                             const uint64_t* dst_offsets, const uint32_t* dst_caps,
                                             uint32_t* d_out_sizes);

/* Greedy packing of unique chunks into stored blocks exactly as Longtail_CreateStoreIndex does it
 * (src/longtail.c:6801-6860: same tag, <= max_chunks_per_block chunks, size <= max_block_size * 1.1).  Host arrays;
 * block_starts[0..*out_block_count] are chunk indices (last entry = chunk_count). */
LTHIP_EXPORT int lthip_pack_blocks(uint64_t chunk_count, const uint32_t* chunk_lens, uint32_t max_block_size,
                                   uint32_t max_chunks_per_block, uint64_t* block_starts, uint64_t capacity,
                                   uint64_t* out_block_count);

/* The same greedy rule, resumable: packs from chunk `first_chunk` until the batch holds max_batch_bytes of chunk data or
 * the blocks' codec bounds (size + size / bound_div + bound_add, rounded up to 64) fill arena_bytes -- always at least one
 * block.  block_starts[0..n] (n = *out_block_count, last entry = *out_next_chunk) and block_sizes[0..n) are host arrays of
 * `capacity` entries.  Lets the caller pack batch k+1 while the device compresses batch k. */
LTHIP_EXPORT int lthip_pack_blocks_batch(uint64_t chunk_count, const uint32_t* chunk_lens, uint64_t first_chunk,
                                         uint32_t max_block_size, uint32_t max_chunks_per_block, uint64_t max_batch_bytes,
                                         uint64_t arena_bytes, uint32_t bound_div, uint32_t bound_add,
                                         uint64_t* block_starts, uint64_t* block_sizes, uint64_t capacity,
                                         uint64_t* out_block_count, uint64_t* out_next_chunk);

/* Block assembly (WriteContentBlockJob, src/longtail.c:4640-4721) as a device gather:
 * d_dst[d_dst_offsets[i] ..) = d_src[d_src_offsets[i] .. + d_lens[i]) for every range (all tables on the device). */
LTHIP_EXPORT int lthip_gather_ranges(lthip_ctx* ctx, const void* d_src, uint64_t range_count, const uint64_t* d_src_offsets,
                                     const uint32_t* d_lens, void* d_dst, const uint64_t* d_dst_offsets);

/* ZStd (ZStdCompressionAPI_Compress, lib/zstd/longtail_zstd.c:105-142): one zstd frame per block, 128 KiB pieces
 * stored as RLE / Compressed (LZ sequences + Huffman literals + FSE) / Raw blocks; decodable by the reference's
 * ZSTD_decompressDCtx.  A compressed piece is a run of small zstd blocks (one per 4 KiB of content, one set of entropy
 * tables per piece) and the frame ends with a skippable frame holding the directory of block sizes, which lets
 * lthip_zstd_decompress_blocks decode every block on a lane of its own (LTHIP_ZSTD_SUB=0: one block per
 * piece).  Same calling convention as lthip_lz4_compress_blocks.  A capacity that holds the frame but not its directory (12 bytes +
 * 2 per 4 KiB of content) gives the frame without it -- still a standard frame, which this library decodes block-parallel like any
 * other encoder's --, a smaller one gives 0. */
LTHIP_EXPORT size_t lthip_zstd_bound(size_t size); /* ZSTD_COMPRESSBOUND, lib/zstd/ext/zstd.h:232 */
LTHIP_EXPORT int lthip_zstd_compress_blocks(lthip_ctx* ctx, const void* d_src, uint32_t block_count,
                                            const uint64_t* src_offsets, const uint32_t* src_sizes, void* d_dst,
                                            const uint64_t* dst_offsets, const uint32_t* dst_caps,
                                            uint32_t* d_out_sizes);
/* The same with the parse the reference's settings ids stand for (lib/zstd/longtail_zstd.c:11-28, 43-60: 'ztd1' -> level 0 = the
 * default 3, 'ztd2' -> 3, 'ztd4' -> 8, 'ztd3' -> 22, 'ztd5' -> its own type id, which zstd clamps to 22; any other id -> 0 = the
 * default, it is NOT rejected there and is not here):
 *   LTHIP_ZSTD_Q_DEFAULT  'ztd1', 'ztd2', unknown ids: the lane parser's greedy parse (what lthip_zstd_compress_blocks runs); a match
 *                         of four bytes must start within 1 KiB, one of five within 4 KiB (the offset's bits are written out: a short
 *                         match from far away costs more than the literals it replaces)
 *   LTHIP_ZSTD_Q_HIGH     'ztd4': every redundant 32 KiB half of a 128 KiB piece but the piece's first is parsed with the 32 KiB in
 *                         front of it as HISTORY (matches reach 32 .. 64 KiB back wherever the half lies; by default a half only sees
 *                         what its 64 KiB group holds in front of it).  About half the match finder's throughput.
 *   LTHIP_ZSTD_Q_MAX      'ztd3', 'ztd5': the history ALSO for a piece's first half -- matches reach into the piece before -- except in
 *                         every eighth piece of a block, and the wave's table is read again after the step's inserts.  The frame's
 *                         trailer says so (directory version 4): this library's decoder runs the eight pieces in between as a CHAIN
 *                         (a piece is executed when the one before it is complete; the chains of a call side by side).  On "tokens"
 *                         2.92 / 3.33 / 3.76 (default / high / max), records 3.00 / 3.12 / 3.24 = the reference encoder's default;
 *                         restore of such frames 0.7-0.9 x the other settings' rate at 512 blocks per call, one block 2-6 ms
 *                         against 0.5-1.4 (profiles/r05_zstd_ratio_table.txt, r05_zstd_quality_rates.txt).
 * Every quality writes standard zstd frames in the sub-block layout; at the first two the pieces of a frame are independent of each
 * other; each is smaller than the one before on the synthetic kinds with structure.
 * lthip_zstd_quality_of_settings: the quality a settings id ('ztd?' as a big-endian u32, the value blocks carry) stands for. */
#define LTHIP_ZSTD_Q_DEFAULT 0
#define LTHIP_ZSTD_Q_HIGH 1
#define LTHIP_ZSTD_Q_MAX 2
LTHIP_EXPORT int lthip_zstd_quality_of_settings(uint32_t settings_id);
LTHIP_EXPORT int lthip_zstd_compress_blocks_q(lthip_ctx* ctx, const void* d_src, uint32_t block_count,
                                              const uint64_t* src_offsets, const uint32_t* src_sizes, void* d_dst,
                                              const uint64_t* dst_offsets, const uint32_t* dst_caps,
                                              uint32_t* d_out_sizes, int quality);
/* ZStdCompressionAPI_Decompress (longtail_zstd.c:144-177): every payload is one or more zstd frames (any encoder's: Huffman /
 * FSE / repeat modes / repeat offsets / skippable frames; no dictionaries; a content checksum is skipped, not verified).
 * d_out_sizes[b] = decoded size, or 0xFFFFFFFF when the payload is malformed or does not fit dst_caps[b]. */
LTHIP_EXPORT int lthip_zstd_decompress_blocks(lthip_ctx* ctx, const void* d_src, uint32_t block_count,
                                              const uint64_t* src_offsets, const uint32_t* src_sizes, void* d_dst,
                                              const uint64_t* dst_offsets, const uint32_t* dst_caps,
                                              uint32_t* d_out_sizes);
/* Diagnostics (tests): what the last lthip_zstd_decompress_blocks call of this process did -- out[0] payloads, out[1] blocks of
 * other encoders' frames that were listed for the block-parallel decoder, out[2] payloads a lane-parallel decoder gave back to the
 * serial one, out[3] where the first of those was sent back (a source line of k_zstd.hip).  Waits for the context's stream. */
LTHIP_EXPORT int lthip_zstd_last_decode_stats(lthip_ctx* ctx, uint32_t out[4]);
/* Tests only: the library caches its environment switches (LTHIP_ZSTD_DBG, LTHIP_LZ4_SERIAL_DECODER, LTHIP_LZ4_DBG, ...) per process; after
 * this call they are read again, so that one process can run a path and its ablation. */
LTHIP_EXPORT void lthip_debug_reload_env(void);
/* Tests only, ABLATION build only (the product library answers ENOTSUP / -1 and has no counter in its allocation path): make the
 * library's own device / pinned allocations number after+1 .. after+count FROM NOW fail with out-of-memory (after < 0: off);
 * lthip_debug_alloc_calls = allocations attempted by this process so far, *out_failed = how many were made to fail.  The device-side
 * counterpart of the reference's FailableStorageAPI tests (test/test.cpp:5677-5752): ENOMEM must come out of CreateVersionIndex /
 * WriteContent, nothing may leak, the same objects must work on the next call. */
LTHIP_EXPORT int lthip_debug_fail_alloc(int64_t after, int64_t count);
LTHIP_EXPORT int64_t lthip_debug_alloc_calls(int64_t* out_failed);
/* Diagnostics, ABLATION build only (the product library answers ENOTSUP): the 4 KiB wave-tiles the walking scans of this process have
 * hashed since the last call.  Waits for the device. */
LTHIP_EXPORT int lthip_debug_walk_tiles(uint64_t* out_tiles);
/* Diagnostics (parity tests): match-finder output of the last lthip_zstd_compress_blocks call (its last internal batch:
 * calls above LTHIP_BATCH_BYTES = 8 GiB of input are processed in several) on this context for the
 * 4 KiB units [first, first + count) -- 16 bytes of meta {nseq, nlit, tail, 0}, 4096 literal bytes and 1024 u64
 * records {lit | mlen << 16 | offset << 32} per unit (host buffers, any may be NULL).  A unit with nseq == 0 has no
 * literal buffer (its 4096 bytes here are unspecified): its literals are its source bytes. */
LTHIP_EXPORT int lthip_zstd_debug_units(lthip_ctx* ctx, uint64_t first, uint64_t count, void* h_meta, void* h_lits,
                                        void* h_recs);

/* ---- dedup (serial first-seen pass of Longtail_CreateVersionIndex, src/longtail.c:2951-2970) --------
 * d_first_index[i] = smallest j with d_hashes[j] == d_hashes[i]; *d_unique_count = number of i with
 * d_first_index[i] == i. */
LTHIP_EXPORT int lthip_dedup_first_seen(lthip_ctx* ctx, uint64_t count, const uint64_t* d_hashes,
                                        uint32_t* d_first_index, uint64_t* d_unique_count);
/* Multi-GPU form: all `count` (all-gathered) hashes go into the table, but only this rank's own range
 * [lookup_first, lookup_first + lookup_count) is answered (d_first_index[j] for hash lookup_first + j, global indices);
 * *d_unique_count = distinct hashes among all `count`. */
LTHIP_EXPORT int lthip_dedup_first_seen_range(lthip_ctx* ctx, uint64_t count, const uint64_t* d_hashes, uint64_t lookup_first,
                                              uint64_t lookup_count, uint32_t* d_first_index, uint64_t* d_unique_count);

/* ---- the first-seen table kept between calls (the stream session's table; k_dedup.hip) -------------------------------------------
 * The same mapping as lthip_dedup_first_seen for an array that arrives in pieces: for ANY way of cutting an array into
 * lthip_seen_add calls, the concatenated d_first_index equals what lthip_dedup_first_seen gives for the whole array.
 *   d_first_index[j] = position, counted over everything added to this table so far (earlier calls first, then this call), of the
 *                      first occurrence of d_hashes[j]: hash j of this call is new  <=>  d_first_index[j] == lthip_seen_total()
 *                      before the call + j
 *   *d_distinct      (device, may be NULL) = distinct hashes in the table after the call
 * The table owns its memory (allocations of its own, not the context's scratch): several tables on one context and one-shot
 * lthip_dedup_first_seen calls in between do not disturb each other.  It holds at least two slots per hash added and grows by
 * re-inserting its (hash, position) pairs into a table of twice the slots; whether a call grows is decided on the host from the
 * running total.  A call that grows may wait for the context's stream, a call that does not never does.  Positions are uint32_t: a
 * total above 0x7FFFFFFF is EINVAL and changes nothing; an allocation that fails while growing is ENOMEM and changes nothing.
 * expected_hashes: the table is created for that many (0: the smallest table, 1024 slots).  Asynchronous on the context's stream;
 * d_hashes must stay valid until the call's work has run.  One table belongs to one context (and its thread). */
typedef struct lthip_seen lthip_seen;
LTHIP_EXPORT int lthip_seen_create(lthip_ctx* ctx, uint64_t expected_hashes, lthip_seen** out);
LTHIP_EXPORT void lthip_seen_destroy(lthip_seen* seen);
LTHIP_EXPORT int lthip_seen_add(lthip_seen* seen, uint64_t count, const uint64_t* d_hashes, uint32_t* d_first_index,
                                uint64_t* d_distinct);
LTHIP_EXPORT uint64_t lthip_seen_total(const lthip_seen* seen); /* hashes added so far: host counter, no synchronisation */
LTHIP_EXPORT uint64_t lthip_seen_grown(const lthip_seen* seen); /* how often the table has grown: host counter */
/* The table as a hash -> position map: d_position[i] = position of the first occurrence of d_hashes[i] among everything added, or
 * 0xFFFFFFFF when the table does not hold it.  Answers what every lthip_seen_add queued before it on the context's stream put in;
 * asynchronous, never waits, changes nothing. */
LTHIP_EXPORT int lthip_seen_find(const lthip_seen* seen, uint64_t count, const uint64_t* d_hashes, uint32_t* d_position);

/* ---- the set of chunk hashes a store already holds (k_dedup.hip) -----------------------------------------------------------------
 * What an upload of version N + 1 into a store that holds versions 1 .. N consults: a device-resident set of 64-bit chunk hashes,
 * built from the store's StoreIndex blobs (lthip_store_add_index) or from device arrays (lthip_store_add), asked with
 * lthip_store_find, and attached to an ingest session with lthip_ingest_stream_set_store / lthip_ingest_set_store -- the session then
 * writes only the chunks the store lacks (Longtail_CreateMissingContent(store, version), src/longtail.c:6882-6998).
 * A key-only open-addressing table: 8 bytes per slot and no position word, so neither lthip_seen's uint32_t positions nor its
 * 2^31 - 1 total apply.  Power-of-two slot count, at least two slots per hash added (duplicates counted: whether a call grows the
 * table is decided on the host from the running total lthip_store_added), growth by re-inserting the keys into a table of at least
 * twice the slots.  The table owns its memory; several stores, lthip_seen tables and one-shot dedup calls on one context do not
 * disturb each other.  One store belongs to one context (and its thread); everything is asynchronous on the context's stream except
 * where stated: a call that grows the table may wait for the stream, lthip_store_distinct does.
 *   create     expected_hashes: the table is created for that many (0: the smallest table, 1024 slots)
 *   add        count device hashes, duplicates (in the call, or of what the store holds) allowed; d_hashes must stay valid until the
 *              call's work has run.  An allocation that fails while growing: ENOMEM, nothing changed, the old table stays live.
 *   add_index  a serialized StoreIndex in HOST memory (the bytes Longtail_WriteStoreIndexToBuffer produces; read before the call
 *              returns): adds its m_ChunkHashes.  EBADF for a blob shorter than its header, another version than 1.0.0 or a
 *              truncated index; the set is unchanged then.
 *   find       d_known[i] = 1 if the store holds d_hashes[i], else 0; *d_known_count (device, may be NULL) is SET to the number of
 *              ones.  Answers what every add queued before it on the context's stream put in.
 *   added      hashes passed to add / add_index so far, duplicates included: host counter, no synchronisation
 *   distinct   distinct hashes in the store; waits for the context's stream
 *   grown      how often the table has grown: host counter */
typedef struct lthip_store lthip_store;
LTHIP_EXPORT int lthip_store_create(lthip_ctx* ctx, uint64_t expected_hashes, lthip_store** out);
LTHIP_EXPORT void lthip_store_destroy(lthip_store* store);
LTHIP_EXPORT int lthip_store_add(lthip_store* store, uint64_t count, const uint64_t* d_hashes);
LTHIP_EXPORT int lthip_store_add_index(lthip_store* store, const void* store_index, size_t store_index_size);
LTHIP_EXPORT int lthip_store_find(const lthip_store* store, uint64_t count, const uint64_t* d_hashes, uint8_t* d_known,
                                  uint64_t* d_known_count);
LTHIP_EXPORT uint64_t lthip_store_added(const lthip_store* store);
LTHIP_EXPORT int lthip_store_distinct(lthip_store* store, uint64_t* out);
LTHIP_EXPORT uint64_t lthip_store_grown(const lthip_store* store);

/* Hash-range-sharded form of the first-seen pass (multi-GPU): this rank holds an arbitrary subset of the tree's chunk hashes, each
 * with its global chunk position; d_first_ordinal[j] = smallest position among the subset's items with the hash of item j.  The
 * ranks route every chunk to the owner of its hash (longtail_amd/dist.py: sharded_first_seen), so a rank inserts 1/N of the tree's
 * chunks instead of all of them. */
LTHIP_EXPORT int lthip_dedup_min_ordinal(lthip_ctx* ctx, uint64_t count, const uint64_t* d_hashes, const uint32_t* d_ordinals,
                                         uint32_t* d_first_ordinal, uint64_t* d_unique_count);

/* ---- bulk Longtail_CreateVersionIndex tail (src/longtail.c:2808-3017, layout :2551-2584, :2709-2806) ---
 * From the device-resident chunk lists of lthip_chunk_hash -- all assets' chunks concatenated in (asset, part, chunk) order,
 * asset a owning asset_chunk_counts[a] of them -- to the SERIALIZED VersionIndex (the bytes Longtail_WriteVersionIndexToBuffer
 * produces, :3415): first-seen unique chunk list + per-asset-chunk indexes, content hash per asset (hash of its chunk-hash
 * array), path hashes.  HASH TYPE: path, content and block hashes of this and the two builders below are BLAKE2s-64 when
 * hash_identifier is 'blk2' (0x626c6b32), Meow-64 when it is 'meow' (0x6d656f77), and BLAKE3-64 for any other identifier ('blk3' and,
 * as before, everything else); the
 * chunk hashes are the caller's and must be of the same type.  The file list is a struct Longtail_FileInfos taken apart (src/longtail.h:1684-1692); directories are
 * assets with zero chunks.  Host arrays unless marked d_.  Returns ENOMEM with *out_size set when `out` is too small. */
LTHIP_EXPORT size_t lthip_version_index_size(uint32_t asset_count, uint64_t unique_chunk_count, uint64_t asset_chunk_index_count,
                                             uint32_t path_data_size);
LTHIP_EXPORT int lthip_build_version_index(lthip_ctx* ctx, uint32_t asset_count, const uint64_t* asset_sizes,
                                           const uint32_t* path_start_offsets, const uint16_t* permissions, const char* path_data,
                                           uint32_t path_data_size, const uint32_t* asset_chunk_counts, uint64_t chunk_total,
                                           const uint64_t* d_chunk_hashes, const uint32_t* d_chunk_lens,
                                           const uint32_t* asset_tags /* may be NULL */, uint32_t hash_identifier,
                                           uint32_t target_chunk_size, void* out, size_t out_capacity, size_t* out_size);

/* ---- stored blocks ------------------------------------------------------------------
 * The bytes of a stored block file (Longtail_WriteStoredBlockToBuffer, src/longtail.c:4111-4150) around a compressed
 * payload: BlockIndex data (block hash = hash of the chunk-hash array :3753-3757, hash identifier, chunk count, tag,
 * chunk hashes, chunk sizes, layout :3585-3601) then [u32 raw size][u32 compressed size] (compressblockstore.c:103-139).
 * Compress block b to  image_offsets[b] + lthip_stored_block_header_size(chunks of b)  first; this call fills in the rest,
 * so the image of block b is  d_arena[image_offsets[b] .. + header size + compressed size).  Block b holds the chunks
 * [block_first_chunk[b], block_first_chunk[b+1]) of the (unique, first-seen ordered) device arrays; image offsets must be
 * 8-byte aligned; host arrays unless marked d_. */
LTHIP_EXPORT size_t lthip_stored_block_header_size(uint32_t chunk_count);
LTHIP_EXPORT int lthip_write_stored_block_headers(lthip_ctx* ctx, uint32_t block_count, const uint64_t* block_first_chunk,
                                                  const uint64_t* d_chunk_hashes, const uint32_t* d_chunk_lens,
                                                  uint32_t hash_identifier, uint32_t tag, const uint32_t* raw_sizes,
                                                  const uint32_t* d_comp_sizes, void* d_arena, const uint64_t* image_offsets);
/* A block with tag 0 is stored RAW: the reference's CompressBlock passes it through (lib/compressblockstore/
 * longtail_compressblockstore.c:85-90), so its file is the BlockIndex followed by the chunks' bytes, without the [raw][compressed] words.
 * lthip_block_index_size(n) = lthip_stored_block_header_size(n) - 8 = 20 + 12 n: the bytes of the BlockIndex; a raw image is that many
 * bytes followed by the raw size of the block's chunks.
 * lthip_write_raw_block_images writes, for every block, the COMPLETE tag-0 image: BlockIndex (block hash of hash_identifier's type, tag 0)
 * + the block's chunks copied from d_src + d_chunk_src_offsets[c] back to back -- byte for byte Longtail_CreateStoredBlock(.., tag 0, ..)
 * + Longtail_WriteStoredBlockToBuffer.  Table conventions as lthip_write_stored_block_headers: block b holds the chunks
 * [block_first_chunk[b], block_first_chunk[b+1]) of the device arrays (hashes, lengths, and here the byte offset of every chunk in
 * d_src); image offsets 8-byte aligned; host arrays unless marked d_ (they may be freed on return).  Asynchronous on the context's
 * stream.  Writes nothing outside [image_offsets[b], + lthip_block_index_size(n_b) + raw_b); reads no 4-byte word of d_src that holds
 * no byte of a chunk (a chunk may end at the last byte of an allocation).  d_src and the arena must not overlap.  Timed as
 * LTHIP_K_GATHER. */
LTHIP_EXPORT size_t lthip_block_index_size(uint32_t chunk_count);
LTHIP_EXPORT int lthip_write_raw_block_images(lthip_ctx* ctx, uint32_t block_count, const uint64_t* block_first_chunk /*host, [n+1]*/,
                                              const uint64_t* d_chunk_hashes, const uint32_t* d_chunk_lens,
                                              const uint64_t* d_chunk_src_offsets, const void* d_src, uint32_t hash_identifier,
                                              void* d_arena, const uint64_t* image_offsets /*host*/);

/* ---- bulk Longtail_CreateMissingContent (src/longtail.c:6882-6998 with DiffHashes :6620-6743 and
 * Longtail_CreateStoreIndex :6745-6880) -------------------------------------------------------------------------------
 * Which of the version's chunks (unique list, version order: device hashes + sizes, host tags or NULL) does a store holding
 * d_existing_hashes lack, and how are they packed into blocks?  Output: the serialized StoreIndex of the missing content
 * (the bytes Longtail_WriteStoreIndexToBuffer produces: blocks with their block hashes -- of hash_identifier's type, see above --,
 * chunk lists, tags).  A chunk list with repeats is outside the contract, here as in the reference; what the reference returns for one
 * (it leaves out chunks that first occur among the list's last entries, src/longtail.c:6666 and :6731) is returned here too, byte for
 * byte.
 * Returns ENOMEM with *out_size set when `out` is too small. */
LTHIP_EXPORT int lthip_create_missing_content(lthip_ctx* ctx, uint64_t existing_count, const uint64_t* d_existing_hashes,
                                              uint64_t chunk_count, const uint64_t* d_chunk_hashes, const uint32_t* d_chunk_lens,
                                              const uint32_t* chunk_tags, uint32_t hash_identifier, uint32_t max_block_size,
                                              uint32_t max_chunks_per_block, void* out, size_t out_capacity, size_t* out_size);

/* ---- bulk Longtail_GetExistingStoreIndex (src/longtail.c:7087-7325) -------------------------------------------
 * Which blocks of a store (its serialized StoreIndex, host memory, the bytes Longtail_WriteStoreIndexToBuffer produces) cover the
 * given chunk hashes (device)?  Blocks are kept when at least min_block_usage_percent of their bytes are wanted, walked most-used
 * first, and taken when they hold a wanted chunk no earlier block of the walk held.  Output: the serialized StoreIndex of the taken
 * blocks (== Longtail_GetExistingStoreIndex + Longtail_WriteStoreIndexToBuffer, including the reference's habit of reading a taken
 * block's tag at its first chunk's index).  Returns ENOMEM with *out_size set when `out` is too small, EBADF for a malformed index. */
LTHIP_EXPORT int lthip_get_existing_store_index(lthip_ctx* ctx, const void* store_index, size_t store_index_size, uint64_t chunk_count,
                                                const uint64_t* d_chunk_hashes, uint32_t min_block_usage_percent, void* out,
                                                size_t out_capacity, size_t* out_size);

/* ---- the ingest metric as one native session (CreateVersionIndex + CreateMissingContent + WriteContent) --------
 * For assets already resident in HBM (a tree that arrives in slices: lthip_ingest_stream_* below).  The caller runs lthip_chunk_hash over its own jobs (one part per job, ascending job order),
 * then
 *   lthip_ingest_index   tail of Longtail_CreateVersionIndex (src/longtail.c:2808-3017: first-seen pass :2951-2970, content hashes
 *                        :2518-2537, path hashes :1269-1300, serialized layout :2551-2584) + Longtail_CreateMissingContent
 *                        (:6882-6998) for the chunks THIS rank writes: packing (:6801-6860), block hashes (:3753-3757)
 *   lthip_ingest_write   Longtail_WriteContent (:4760; WriteContentBlockJob :4559-4758, CompressBlock compressblockstore.c:67-141):
 *                        block assembly on the device only for blocks that are not one byte range of the data, per-block codec
 *                        straight into the stored-block image, BlockIndex + [raw][compressed] around it (:4111-4150).  The images
 *                        are produced batch after batch in the caller's arena and dropped (null sink).
 *   lthip_ingest_finish  serialized StoreIndex of what was written (:8913-8931), the session's one full synchronisation, statistics.
 * Single GPU: the "all" arrays are the local ones and tree->my_jobs is NULL.  Multi-GPU: the "all" arrays hold every rank's
 * chunks in job order (see lthip_exchange_layout) and tree->my_jobs lists this rank's jobs; a rank writes the chunks that are
 * first-seen and lie in its own jobs, i.e. Longtail_CreateMissingContent against a store that already holds the other ranks'
 * chunks.  h_version_index (may be NULL: this rank does not serialize the index) and h_store_index should be pinned memory so
 * the copies overlap the kernels.  asset_tags NULL = every asset carries cfg.compression_type (what UpSync passes).
 * Lifetimes.  The host arrays of `tree` (sizes, paths, permissions, tags, job tables) may be freed or reused as soon as
 * lthip_ingest_index has returned (the session keeps its own copy of what it reads later: round 4; round 3 read the caller's arrays from
 * a helper thread until lthip_ingest_finish).  The DEVICE arrays (d_all_hashes, d_all_lens, d_local_*) and the VersionIndex buffer must
 * stay valid, and the buffer unread, until lthip_ingest_finish has returned: the index is serialized by a helper thread next to
 * lthip_ingest_write, and the packing into blocks is finished there too (the result's block count comes from lthip_ingest_finish).
 * TAGS AND CODECS (both sessions).  Blocks are packed by tag and every index records the tags; cfg.codec says what is written:
 *   LTHIP_CODEC_BY_TAG  every block's codec follows its own tag, as in the reference (compressblockstore.c:85-97):
 *                         0                  a raw image: BlockIndex + the chunks' bytes (lthip_block_index_size)
 *                         'lz42'             LZ4
 *                         'ztd1' .. 'ztd5'   zstd at lthip_zstd_quality_of_settings(tag)
 *                       Any other tag (the 'btl?' ids included) is ENOTSUP.
 *   LTHIP_CODEC_NONE    all blocks are written raw.  Valid only when every tag is 0: cfg.compression_type == 0, and asset_tags NULL
 *                       or all zero; EINVAL otherwise.
 *   LTHIP_CODEC_LZ4 / LTHIP_CODEC_ZSTD   ONE codec for all blocks whatever their tags (zstd at the quality of cfg.compression_type):
 *                       the caller vouches that every tag names that codec -- a reader picks the decoder by the tag.
 * The refusals come before any work is queued and leave the context and the session usable.  cfg.compression_type -- the single tag
 * when asset_tags == NULL -- is checked by lthip_ingest_create and lthip_ingest_stream_create (always: with asset tags it must still be
 * a tag the mode takes, 0 will do); the asset tags by lthip_ingest_index and lthip_ingest_stream_create.
 * A raw block counts its raw size in compressed_bytes and in lthip_ingest_compressed_sizes; its image is lthip_block_index_size(n) + raw
 * bytes long.  Raw blocks are copied straight from where their chunks lie: they never go through the block assembly and count 0 in
 * gathered_blocks / gathered_bytes. */
enum lthip_codec
{
    LTHIP_CODEC_NONE = 0,
    LTHIP_CODEC_LZ4 = 1,
    LTHIP_CODEC_ZSTD = 2,
    LTHIP_CODEC_BY_TAG = 3
};
typedef struct lthip_ingest lthip_ingest;
typedef struct lthip_ingest_config
{
    uint32_t target_chunk_size;    /* recorded in the VersionIndex */
    uint32_t hash_identifier;      /* 0x626c6b33 'blk3', 0x626c6b32 'blk2': path / content / block hashes with BLAKE2s (the caller's
                                      chunk hashes then come from lthip_blake2s_ranges[_dev]), or 0x6d656f77 'meow': with Meow
                                      (chunk hashes from lthip_meow_ranges[_dev]); any other value hashes with BLAKE3 */
    uint32_t max_block_size;       /* cmd/main.c:3006-3009 defaults: 8 MiB */
    uint32_t max_chunks_per_block; /*                                 1024  */
    uint32_t compression_type;     /* the tag stored with chunks and blocks: 0 (raw), 'lz42', 'ztd1'..'ztd5' */
    uint32_t codec;                /* enum lthip_codec */
    uint64_t batch_bytes;          /* raw bytes per codec batch, 0 = 8 GiB */
} lthip_ingest_config;
typedef struct lthip_ingest_tree
{
    uint32_t asset_count;               /* struct Longtail_FileInfos taken apart (src/longtail.h:1684-1692) */
    const uint64_t* asset_sizes;
    const uint32_t* path_start_offsets;
    const uint16_t* permissions;
    const char* path_data;
    uint32_t path_data_size;
    const uint32_t* asset_tags;         /* may be NULL */
    uint64_t job_count;                 /* lthip_make_jobs */
    const uint32_t* job_asset;
    const uint64_t* job_first;          /* [job_count + 1] index of each job's first chunk in the "all" arrays */
    uint64_t my_job_count;
    const uint64_t* my_jobs;            /* ascending job indices of this rank; NULL = all jobs */
} lthip_ingest_tree;
typedef struct lthip_ingest_result
{
    uint64_t struct_size;                 /* IN: sizeof(lthip_ingest_result) of the caller's header; the library fills at most that */
    uint64_t chunks_all, unique_all;      /* chunks / distinct chunks of the whole tree */
    uint64_t chunks_local, unique_local;  /* chunks of this rank's jobs / those of them this rank writes */
    uint64_t blocks, raw_bytes, compressed_bytes, gathered_blocks;
    uint64_t version_index_size, store_index_size;
    uint64_t gathered_bytes;              /* bytes of the blocks that went through the device block assembly */
} lthip_ingest_result;
LTHIP_EXPORT int lthip_ingest_create(lthip_ctx* ctx, const lthip_ingest_config* config, lthip_ingest** out);
LTHIP_EXPORT void lthip_ingest_destroy(lthip_ingest* ingest);
LTHIP_EXPORT int lthip_ingest_index(lthip_ingest* ingest, const lthip_ingest_tree* tree, const uint64_t* d_all_hashes,
                                    const uint32_t* d_all_lens, uint64_t all_chunks, const uint64_t* d_local_offsets,
                                    const uint32_t* d_local_part_first, uint64_t local_chunks, void* h_version_index,
                                    size_t version_index_capacity);
/* Multi-GPU with the hash-range-sharded first-seen table: d_first_index[i] = position of the first chunk (job order, all ranks) with
 * the hash of chunk i, for all `all_chunks` chunks of the NEXT lthip_ingest_index call, and the tree's number of distinct hashes; that
 * call then skips its own table pass (every rank inserting every rank's hashes).  The array must stay valid until the call returns. */
LTHIP_EXPORT int lthip_ingest_set_first_seen(lthip_ingest* ingest, const uint32_t* d_first_index, uint64_t unique_chunks);
LTHIP_EXPORT int lthip_ingest_write(lthip_ingest* ingest, const void* d_data, void* d_arena, uint64_t arena_bytes);
LTHIP_EXPORT int lthip_ingest_finish(lthip_ingest* ingest, void* h_store_index, size_t store_index_capacity,
                                     lthip_ingest_result* out_result);
/* The stored-block images of the LAST codec batch of lthip_ingest_write (host tables owned by the session, valid after
 * lthip_ingest_finish until the next lthip_ingest_index): blocks *out_first_block .. + *out_count of the session; image i lies at
 * d_arena + offsets[i] and is sizes[i] bytes long -- BlockIndex, [raw size][compressed size], payload (a raw block: BlockIndex, the
 * chunks' bytes): exactly what
 * Longtail_WriteStoredBlockToBuffer produces and PutStoredBlock receives (src/longtail.c:4111-4150, 4722-4757).  A session whose
 * write fit ONE batch (raw bytes <= cfg.batch_bytes, and the arena) has all of its images there: the host-fed loop of INTEGRATION.md
 * (pinned slice -> H2D -> lthip_chunk_hash -> session -> images D2H) downloads them through this table. */
LTHIP_EXPORT int lthip_ingest_images(const lthip_ingest* ingest, uint64_t* out_first_block, uint64_t* out_count,
                                     const uint64_t** out_offsets, const uint32_t** out_sizes);
/* per-block compressed sizes of the last lthip_ingest_write (host, valid after lthip_ingest_finish) */
LTHIP_EXPORT const uint32_t* lthip_ingest_compressed_sizes(const lthip_ingest* ingest);
/* Uploading into a store that already has content: with a store attached, the following lthip_ingest_index calls write only the
 * chunks the store lacks -- a rank writes the chunks that are first-seen, lie in its own jobs AND are unknown to the store.  The
 * VersionIndex is unchanged (the whole version's); the StoreIndex is Longtail_CreateMissingContent(store, version) for a single rank,
 * and for R ranks that all hold the same store the reference's with existing = store + the chunks first seen in other ranks' jobs.
 * When nothing is missing the StoreIndex is the 16-byte header of Longtail_CreateStoreIndexFromBlocks(0, 0) (hash identifier 0,
 * src/longtail.c:6931-6943).  Result: unique_all = the version's distinct chunks, unique_local / blocks / raw_bytes / compressed_bytes
 * what this rank wrote.  The store must be of the session's context and must not be added to or destroyed between lthip_ingest_index
 * and lthip_ingest_finish; NULL detaches it.  lthip_ingest_store_stats (after lthip_ingest_index): the first-seen chunks of this
 * rank's own jobs that the store held, and their bytes; 0 / 0 without a store. */
LTHIP_EXPORT int lthip_ingest_set_store(lthip_ingest* ingest, const lthip_store* store);
LTHIP_EXPORT int lthip_ingest_store_stats(const lthip_ingest* ingest, uint64_t* known_chunks, uint64_t* known_bytes);

/* ---- the ingest session for a tree that arrives in slices (ingest_stream.hip) ----------------------------------------------------
 * lthip_ingest_index / _write / _finish need the whole tree's chunk lists and bytes on the device.  This session takes the tree as
 * SLICES -- contiguous runs of jobs in job order, cut anywhere, inside an asset too -- and still delivers ONE index pair: after
 * lthip_ingest_stream_finish
 *   the VersionIndex  is the bytes of Longtail_CreateVersionIndex + Longtail_WriteVersionIndexToBuffer for the tree,
 *   the StoreIndex    is the bytes of Longtail_CreateMissingContent against an empty store for the version's unique chunks: the
 *                     packing rule of src/longtail.c:6801-6860 applied to the unique list of the WHOLE tree, wherever the cuts fell
 *                     (against the attached store, if there is one: lthip_ingest_stream_set_store below),
 *   the images        of all slice calls and of finish, in call order, are the blocks of that StoreIndex in its order (BlockIndex +
 *                     [raw][compressed] + payload, as lthip_ingest_images delivers them).
 * One first-seen table (lthip_seen) lives for the session: a chunk is written if it is new in its slice's lthip_seen_add, with its
 * asset's tag.  At the end of a slice exactly one block may be open (its successor chunk has not been seen): its chunk list stays
 * with the session and its BYTES are gathered into a session-owned device buffer of max_block_size * 1.1 bytes, as part of the work
 * the slice call queues; the next slice's call assembles the block from those bytes plus its own chunks.
 *
 *   create   tree: the assets (sizes, paths, permissions, tags or NULL) and the job table (job_count, job_asset) of lthip_make_jobs,
 *            deep-copied; job_first is ignored; my_jobs must be NULL (single GPU), EINVAL otherwise.  cfg.codec: any enum lthip_codec, with the tag rules
 *            of TAGS AND CODECS above (ENOTSUP / EINVAL for tags the codec mode does not take).
 *            No chunk may be larger than a block, L = max_block_size * 1.1 (the open block's buffer and the arena bound hold L):
 *            EINVAL when the chunker's largest chunk, max(48, 2 * target_chunk_size), exceeds L; a slice whose lists hold a larger
 *            chunk all the same (another chunker) fails with EINVAL.
 *   slice    jobs [first_job, first_job + job_count): d_data and the four lists are what lthip_chunk_hash produced for a plan of
 *            exactly these jobs, one part per job, ascending (d_part_first has job_count + 1 entries, chunks = its last).  The call
 *            waits once, for the lists to reach the host (the packing is the host's); it does not wait for the codec -- as long
 *            as the call's host tables fit the context's staging slots: eight tables above 64 KiB are in flight at a time, so a
 *            call that closes more than 8192 blocks, or gathers the open block in more than 8192 ranges, reuses a slot whose
 *            upload was queued behind the codec and waits for it.
 *   images   the images the LAST slice (or finish) call produced, in d_arena of that call; waits for that call's work.  Same shape
 *            as lthip_ingest_images; the tables are the session's and valid until its next call.
 *   finish   closes the open block into d_arena, then serializes both indexes of the WHOLE tree (h_version_index / h_store_index may
 *            be NULL: sizes only).  A buffer that is too small: ENOMEM with both sizes in the result, nothing done, call again.
 *            Idempotent like lthip_ingest_finish.  The result is filled as there (struct_size honoured), chunks_local = chunks_all
 *            and unique_local = unique_all.
 * LIFETIMES.  Once the work a slice call queued has run -- lthip_ingest_stream_images has returned, or the context was synchronised
 * -- the caller may overwrite d_data and the four lists, and, having read the images, the arena: the session reads none of them
 * again.  The tree's host arrays may be freed when create has returned.
 * THE ARENA.  lthip_ingest_stream_arena_bound is host arithmetic only: an arena of that many bytes holds the images of ANY slice of
 * slice_bytes bytes in slice_chunks chunks, the block carried in from the slice before included (an image slot is
 * round64(lthip_stored_block_header_size(n) + codec bound(raw)), as in lthip_ingest_write; with LTHIP_CODEC_NONE a slot is
 * round64(lthip_block_index_size(n) + raw), with LTHIP_CODEC_BY_TAG a slot is the largest of the three codecs' slots, so the bound is no less than any one codec's).  A slice call with fewer arena_bytes
 * returns ENOMEM before it touches the session; finish needs lthip_ingest_stream_arena_bound(cfg, 0, 0).
 * ERRORS.  Refused before any work, the session stays usable: a slice that does not start at the next expected job (EINVAL), a call
 * after finish (EINVAL), finish before the last job (EINVAL), an arena below the bound (ENOMEM).  Any failure after work has started
 * makes the session return that errno from every later call except destroy. */
typedef struct lthip_ingest_stream lthip_ingest_stream;
LTHIP_EXPORT int lthip_ingest_stream_create(lthip_ctx* ctx, const lthip_ingest_config* config, const lthip_ingest_tree* tree,
                                            lthip_ingest_stream** out);
LTHIP_EXPORT void lthip_ingest_stream_destroy(lthip_ingest_stream* stream);
LTHIP_EXPORT size_t lthip_ingest_stream_arena_bound(const lthip_ingest_config* config, uint64_t slice_bytes, uint64_t slice_chunks);
LTHIP_EXPORT int lthip_ingest_stream_slice(lthip_ingest_stream* stream, uint64_t first_job, uint64_t job_count, const void* d_data,
                                           const uint64_t* d_chunk_offsets, const uint32_t* d_chunk_lens,
                                           const uint64_t* d_chunk_hashes, const uint32_t* d_part_first, uint64_t chunks,
                                           void* d_arena, uint64_t arena_bytes);
LTHIP_EXPORT int lthip_ingest_stream_images(lthip_ingest_stream* stream, uint64_t* out_first_block, uint64_t* out_count,
                                            const uint64_t** out_offsets, const uint32_t** out_sizes);
LTHIP_EXPORT int lthip_ingest_stream_finish(lthip_ingest_stream* stream, void* d_arena, uint64_t arena_bytes, void* h_version_index,
                                            size_t version_index_capacity, void* h_store_index, size_t store_index_capacity,
                                            lthip_ingest_result* out_result);
/* how often the session's first-seen table has grown so far (lthip_seen_grown of it) */
LTHIP_EXPORT uint64_t lthip_ingest_stream_table_grown(const lthip_ingest_stream* stream);
/* Uploading into a store that already has content.  set_store is allowed before the first slice call (EINVAL afterwards, the session
 * stays usable); the store must be of the session's context; NULL detaches it.  With a store attached a slice asks it about the
 * slice's hashes (lthip_store_find, queued beside the first-seen pass; one more byte per chunk comes to the host in the call's one
 * wait) and a chunk is written only if it is new in the session's table AND unknown to the store.  After finish
 *   the VersionIndex  is unchanged: the reference's bytes for the tree,
 *   the StoreIndex    is the bytes of Longtail_CreateMissingContent(store, version) + Longtail_WriteStoreIndexToBuffer: the packing
 *                     of :6801-6860 over the version-unique chunks the store lacks, in version order, with their assets' tags,
 *                     wherever the cuts fell; when no chunk is missing, the 16-byte header with zero blocks and zero chunks
 *                     (hash identifier 0, :6931-6943) and no images,
 *   the images        of all calls, in call order, are that StoreIndex's blocks,
 *   the result        unique_all = the version's distinct chunks, unique_local = the chunks written; raw_bytes, compressed_bytes and
 *                     blocks count what was written (without a store unique_local == unique_all).
 * lthip_ingest_stream_arena_bound stays an upper bound (fewer chunks are packed).  Adding to an attached store between the first
 * slice and finish is not supported; the store must outlive the session's last slice call.
 * lthip_ingest_stream_store_stats: the version-unique chunks (so far) that the store held, and their bytes; 0 / 0 without a store. */
LTHIP_EXPORT int lthip_ingest_stream_set_store(lthip_ingest_stream* stream, const lthip_store* store);
LTHIP_EXPORT int lthip_ingest_stream_store_stats(const lthip_ingest_stream* stream, uint64_t* known_chunks, uint64_t* known_bytes);

/* ---- the restore session: stored blocks back into a version's assets (restore.hip, restore_call.h) ----------------------------------
 * The device side of Longtail_WriteVersion (src/longtail.c:6471-6573 with BuildAssetWriteList :6021 and WriteAssetsFromBlock :5700) and
 * of DecompressBlock (compressblockstore.c:271-338) for a caller that holds a serialized VersionIndex, a serialized StoreIndex and the
 * stored-block images the ingest sessions (or the reference) wrote, the images already in HBM: the assets' bytes are written into ONE
 * device buffer, asset a at asset_offsets[a].  Single GPU; files are not written.
 *   layout         host only.  The dense layout of a serialized VersionIndex's assets: asset_offsets[a] (may be NULL) = the end of asset
 *                  a - 1 rounded up to `align` (a power of two, >= 1; EINVAL otherwise), *total_bytes = the end of the last asset,
 *                  *asset_count = the version's assets.  EBADF for a blob that is short, of another version than 0.0.2, or inconsistent
 *                  (a chunk index that names no chunk, an asset whose chunk sizes do not sum to its size, a path that does not end
 *                  inside the blob, a hash identifier other than 'blk2' / 'blk3' / 'meow', a target chunk size of 2^31 or more).
 *   create         reads both blobs (host memory, any alignment; they may be freed on return) and asset_offsets[asset_count] (host): any
 *                  byte offsets into the output, no alignment required, LTHIP_RESTORE_SKIP leaves the asset out.  Builds the write plan
 *                  on the device -- per selected asset and chunk one OCCURRENCE (chunk hash, destination, length), resolved against
 *                  the StoreIndex's chunk hashes in an lthip_seen of the session's own and sorted block-major -- and waits for the
 *                  stream once, for the plan's per-block counts.  EBADF: a malformed blob.  EINVAL: the blobs' hash identifiers differ
 *                  (a StoreIndex without chunks has none), or a selected asset's window leaves [0, out_bytes).  ENOENT: a selected asset
 *                  needs a chunk the StoreIndex does not hold (src/longtail.c:6081, :6094) or holds with another size.  ENOMEM.  On any
 *                  error nothing stays allocated and the context stays usable.  Directories and empty files plan nothing; content and
 *                  path hashes are not consulted.  cfg->verify: 1 = every chunk of a delivered block is hashed and compared.
 *   needed_blocks  host only.  The blocks that hold a chunk of a selected asset, in StoreIndex order; block_hashes NULL or capacity too
 *                  small: the count only.
 *   scratch_bound  host arithmetic: the scratch a blocks call with these blocks needs -- round64(raw size) per needed block with a
 *                  codec's tag, 0 for raw (tag 0) blocks, unneeded blocks and hashes the StoreIndex does not hold.
 *   blocks         delivers block_count images: image i lies at d_images + image_offsets[i] (8-byte aligned, EINVAL otherwise) and is
 *                  image_sizes[i] bytes long.  Refused before any work is queued, the session unchanged and usable: ENOENT a block hash
 *                  the StoreIndex does not hold, EEXIST a block delivered before or twice in the call, ENOTSUP a needed block whose tag
 *                  names no codec here ('btl?' ...), ENOMEM scratch below the bound.  A block no selected asset needs is accepted,
 *                  counted and not touched.  Everything else is queued on the context's stream: the call never waits for the device
 *                  (but where a scratch pool of the context has to grow, as in every bulk call, and for a BLAKE3 verify of chunks
 *                  above 256 KiB, whose launcher reads a count back) and reads nothing back -- every decoder table comes from the
 *                  StoreIndex and image_sizes: raw size = the sum of the block's chunk sizes, compressed size = image size -
 *                  lthip_stored_block_header_size(n).  Queued per call:
 *                    check    a wave per image compares block hash, hash identifier, chunk count, tag, every chunk hash and size, and
 *                             for a tagged block the [raw][compressed] words, against the session's device copy of the StoreIndex; it
 *                             reads nothing beyond image_sizes[i]; an image shorter than its header is bad
 *                    decode   tagged blocks through lthip_lz4_decompress_blocks / lthip_zstd_decompress_blocks, one call per codec, into
 *                             64-byte slots of d_scratch.  Both decoders take a payload at ANY byte position (they load the source by
 *                             dwords around it, k_lz4_decode.hip / zd_execute.inc), so the payload -- 28 + 12 n bytes into an 8-byte
 *                             aligned image, i.e. 4-byte aligned -- is decoded where it lies: the session does not realign it.  A raw
 *                             block is not copied: its chunks lie at image + lthip_block_index_size(n)
 *                    verify   (cfg.verify) the chunks of the good blocks hashed with the StoreIndex's hash type and compared
 *                    scatter  every planned occurrence of the call's good blocks copied to its destination: 16-byte stores, source and
 *                             destination at any, independent byte positions; no 4-byte word is read that holds no byte of the chunk (a
 *                             chunk may end at the last byte of d_scratch or of an image).  Timed as LTHIP_K_GATHER (the decoders and
 *                             the hashes as they always are, everything else as LTHIP_K_OTHER)
 *                  d_images and d_scratch may be reused once the call's work has run.  The scatter, and a decoder's second pass, cost
 *                  one more read and write of the output than a decoder writing into place would (first figures: README.md, "Restore
 *                  session"; tools/restore_rate.py).
 *   finish         the session's one full synchronisation.  0: every needed block was delivered and good.  ENOENT: needed blocks are
 *                  outstanding (result.blocks_needed - the needed ones delivered); deliver more and call again.  EBADF: a delivered
 *                  block was bad -- it takes precedence.  The result is filled either way (struct_size honoured).
 *   block_status   after finish: per block hash 0 or flag bits; ENOENT for a hash the StoreIndex does not hold.
 * THE GUARANTEE: no byte of a bad block reaches d_out, and nothing is written outside the selected assets' windows.  A block is bad
 * when its header differs from the StoreIndex (LTHIP_RESTORE_BAD_HEADER), when its decoder does not return exactly the raw size -- a
 * raw image that is not lthip_block_index_size(n) + raw size bytes long counts as that -- (LTHIP_RESTORE_BAD_PAYLOAD), or, with verify,
 * when one of its chunks does not hash to its recorded hash (LTHIP_RESTORE_BAD_CHUNK).  The payload behind a wrong header is not
 * judged: such a block carries LTHIP_RESTORE_BAD_HEADER alone.  The occurrences a bad block feeds keep what d_out held.  One session belongs to one context (and its thread) and must be destroyed before it. */
#define LTHIP_RESTORE_SKIP 0xFFFFFFFFFFFFFFFFull
#define LTHIP_RESTORE_NOT_DELIVERED 1u
#define LTHIP_RESTORE_BAD_HEADER 2u
#define LTHIP_RESTORE_BAD_PAYLOAD 4u
#define LTHIP_RESTORE_BAD_CHUNK 8u
typedef struct lthip_restore lthip_restore;
typedef struct lthip_restore_config
{
    uint64_t struct_size; /* IN: sizeof(lthip_restore_config) of the caller's header; the library reads at most that */
    uint32_t verify;      /* 0 or 1 */
} lthip_restore_config;
typedef struct lthip_restore_result
{
    uint64_t struct_size;       /* IN: sizeof(lthip_restore_result) of the caller's header; the library fills at most that */
    uint64_t assets_selected;   /* assets with an offset other than LTHIP_RESTORE_SKIP; create_windows: distinct assets a window names */
    uint64_t occurrences;       /* planned chunk writes */
    uint64_t occurrences_written, bytes_written; /* those fed by delivered, good blocks and, once carried, by good chunks of the base */
    uint64_t blocks_needed, blocks_delivered /* all accepted blocks, unneeded ones included */, blocks_unneeded, blocks_bad;
    uint64_t chunks_mismatched; /* verify: chunks whose hash differed */
    uint64_t decoded_bytes;     /* raw bytes of the tagged blocks whose decoder returned the raw size */
    uint64_t base_occurrences, base_bytes; /* of the planned writes, those the base feeds (0 without a base) */
    uint64_t base_chunks_mismatched;       /* verify: distinct base chunks whose hash differed */
} lthip_restore_result;
LTHIP_EXPORT int lthip_restore_layout(const void* version_index, size_t version_index_size, uint64_t align, uint64_t* asset_offsets,
                                      uint32_t* asset_count, uint64_t* total_bytes);
LTHIP_EXPORT int lthip_restore_create(lthip_ctx* ctx, const lthip_restore_config* config, const void* version_index,
                                      size_t version_index_size, const void* store_index, size_t store_index_size,
                                      const uint64_t* asset_offsets /*host, [asset_count]*/, uint64_t out_bytes, lthip_restore** out);
LTHIP_EXPORT void lthip_restore_destroy(lthip_restore* restore);
LTHIP_EXPORT int lthip_restore_needed_blocks(const lthip_restore* restore, uint64_t* block_hashes, uint64_t capacity, uint64_t* out_count);
LTHIP_EXPORT size_t lthip_restore_scratch_bound(const lthip_restore* restore, uint32_t block_count, const uint64_t* block_hashes);
LTHIP_EXPORT int lthip_restore_blocks(lthip_restore* restore, uint32_t block_count, const uint64_t* block_hashes /*host*/,
                                      const void* d_images, const uint64_t* image_offsets /*host, 8-byte aligned*/,
                                      const uint32_t* image_sizes /*host*/, void* d_scratch, uint64_t scratch_bytes, void* d_out);
LTHIP_EXPORT int lthip_restore_finish(lthip_restore* restore, lthip_restore_result* out_result);
LTHIP_EXPORT int lthip_restore_block_status(const lthip_restore* restore, uint32_t count, const uint64_t* block_hashes, uint32_t* status);

/* ---- updating a resident version: a base for the restore session (restore.hip) ------------------------------------------------------
 * The device side of the reference's down-sync -- Longtail_GetRequiredChunkHashes (src/longtail.c:4349-4418) and the copying half of
 * Longtail_ChangeVersion (:8013) -- for a caller in whose HBM version N lies restored while version N + 1 is wanted: the chunks the two
 * share are copied from where they lie, and only the rest has to come out of delivered blocks.  The StoreIndex may then be the small
 * one an incremental ingest returns (lthip_ingest*_set_store: the blocks N + 1 added), which lthip_restore_create refuses with ENOENT.
 *   create_from_base  lthip_restore_create with a second source.  base->version_index: the serialized VersionIndex of the resident
 *                  version (host, any alignment, may be freed on return); base->asset_offsets[a]: asset a of the base lies at
 *                  d_base + asset_offsets[a], LTHIP_RESTORE_SKIP = not resident; every resident asset's window lies in
 *                  [0, base->base_bytes).  An occurrence of the target is FED BY THE BASE when the base holds its chunk hash with the
 *                  same size in a resident asset (the first such place, in asset and chunk order); otherwise it is resolved against the
 *                  StoreIndex exactly as lthip_restore_create does; ENOENT when neither holds it.  The base wins when both hold a chunk:
 *                  needed_blocks shrinks to the blocks that hold a chunk no resident asset has, and needed_blocks, scratch_bound,
 *                  blocks and block_status work unchanged over that shorter list.  Still one read-back and one wait.  EINVAL: base or
 *                  base->version_index is NULL, base->struct_size is not sizeof(lthip_restore_base), the hash identifiers of base and
 *                  target differ, a resident base asset's window leaves [0, base_bytes).  EBADF: the base blob is malformed.  Every
 *                  other refusal as lthip_restore_create; on any error nothing stays allocated and the context stays usable.
 *   carry          queues the copy of every base-fed occurrence from d_base to d_out on the context's stream: never waits, reads nothing
 *                  back, allocates nothing (but where a scratch pool of the context has to grow, and for a BLAKE3 verify of chunks
 *                  above 256 KiB, as blocks).  The base-fed occurrences are kept in occurrence order (asset by asset, chunk by chunk);
 *                  an entry that continues the one before it in source AND destination joins its run, and maximal runs are copied by
 *                  the raw-block copy (k_raw_copy) in pieces of 32 KiB: an unchanged asset, and an unchanged stretch of a modified one,
 *                  is one run.  Source and destination at any byte positions; no 4-byte word is read that holds no byte of a chunk.
 *                  cfg.verify: before the copy the base chunks that feed something are hashed where they lie in d_base, with the
 *                  VersionIndex's hash type, and compared with the base VersionIndex's hashes; a chunk that differs is counted and every
 *                  occurrence it would have fed is left out and keeps what d_out held -- THE GUARANTEE extended to the base.  WITHOUT
 *                  verify THE BASE IS TRUSTED and copied as it is.  EINVAL: the session has no base; d_base or d_out is NULL while
 *                  there are base-fed occurrences; [d_base, d_base + base_bytes) and [d_out, d_out + out_bytes) overlap (the update is
 *                  out of place).  EEXIST: carry was called before.  A refused call changes nothing.  carry and the blocks calls write
 *                  disjoint destinations and may come in any order; d_base must stay valid and unchanged until the work has run.
 *   finish         additionally ENOENT while base-fed occurrences exist and carry has not been called, EBADF (it keeps precedence)
 *                  for a mismatched base chunk.  result.occurrences stays every planned write; base_occurrences / base_bytes are those
 *                  planned from the base; occurrences_written / bytes_written count both sources and exclude what a mismatched base
 *                  chunk would have fed. */
typedef struct lthip_restore_base
{
    uint64_t struct_size;          /* IN: sizeof(lthip_restore_base) */
    const void* version_index;     /* the serialized VersionIndex of the version that is resident (host, any alignment) */
    uint64_t version_index_size;
    const uint64_t* asset_offsets; /* host, [its asset count]: asset a of the base lies at d_base + asset_offsets[a];
                                      LTHIP_RESTORE_SKIP = not resident */
    uint64_t base_bytes;           /* every resident asset's window lies in [0, base_bytes) */
} lthip_restore_base;
LTHIP_EXPORT int lthip_restore_create_from_base(lthip_ctx* ctx, const lthip_restore_config* config, const lthip_restore_base* base,
                                                const void* version_index, size_t version_index_size, const void* store_index,
                                                size_t store_index_size, const uint64_t* asset_offsets /*host, [asset_count]*/,
                                                uint64_t out_bytes, lthip_restore** out);
LTHIP_EXPORT int lthip_restore_carry(lthip_restore* restore, const void* d_base, void* d_out);
/* What changed between two serialized VersionIndexes, host only (version_diff.h): the lists of Longtail_CreateVersionDiff
 * (src/longtail.c:7493-7756).  Assets are matched by path hash.  source_removed[source assets] / target_added[target assets]: asset
 * indices only one version has; the content-modified and permissions-modified pairs [min of both asset counts]: an asset both have
 * whose content hashes / permissions differ (it may be in both pairs), source and target index at the same position, in ascending
 * path-hash order, identical with the reference's.  Removed assets are ordered by path length, longest first, added ones shortest first;
 * the reference leaves assets of equal path length to its qsort, here they stay in ascending path-hash order.  Any list pointer may be
 * NULL; counts[4] = {removed, added, modified content, modified permissions} is always filled.  EBADF: a malformed blob, or two assets
 * of one version with the same path hash.  EINVAL: a NULL blob or counts, or the hash identifiers differ.  The restore session does not
 * call it: it is what lets a caller restore only what changed (LTHIP_RESTORE_SKIP for every target asset outside target_added and
 * target_content_modified) and tells it which files to delete or re-permission. */
LTHIP_EXPORT int lthip_version_diff(const void* source_version_index, size_t source_size, const void* target_version_index, size_t target_size,
                                    uint32_t* source_removed, uint32_t* target_added, uint32_t* source_content_modified,
                                    uint32_t* target_content_modified, uint32_t* source_permissions_modified,
                                    uint32_t* target_permissions_modified, uint32_t counts[4]);

/* ---- updating a resident version in place (restore.hip, restore_layout.h) -------------------------------------------------------------
 * Longtail_ChangeVersion (src/longtail.c:8013) works in place: it leaves unchanged files alone and rewrites the rest.  This is its
 * device side.  The base's and the target's asset offsets are offsets into ONE buffer d_buf of max(base_bytes, out_bytes) bytes; the
 * session is created with lthip_restore_create_from_base as before.  An update then costs what changed, not what the version weighs.
 *   layout_in_place  host only.  Assets are matched by path hash.  A target asset of size > 0 is KEPT when the base has a resident asset
 *                  (offset != LTHIP_RESTORE_SKIP) with the same path hash, size and content hash: it gets that asset's offset.  The
 *                  GAPS are [0, base_bytes) minus the kept windows, ascending, each with a cursor at its start.  Every other target
 *                  asset of size > 0, in asset order, goes into the first gap where round_up(cursor, align) + size <= the gap's end, and
 *                  the cursor moves to its end; one that fits no gap is appended at round_up(end, align), `end` starting at base_bytes.
 *                  Assets of size 0 and directories get offset 0.  *total_bytes: the highest end of any target window (it may lie
 *                  below base_bytes); *kept_assets: how many were kept.  Every output may be NULL.  New assets deliberately land on the
 *                  old bytes of modified ones: carry_in_place makes that safe.  EBADF: a malformed blob, or two assets of one version
 *                  with the same path hash.  EINVAL: align is no power of two, a NULL blob or NULL base_offsets, the hash identifiers
 *                  differ, a resident base asset leaves [0, base_bytes), two kept windows overlap.
 *   carry_in_place  a base-fed entry of the plan whose source offset equals its destination is KEPT: nothing is queued for it.  Every
 *                  other one is MOVED (a base chunk's place is its FIRST place in the base, so a duplicate chunk inside an unchanged
 *                  asset can count as moved although its bytes are right; in_place_stats shows it).  Maximal runs are built as carry
 *                  builds them -- a run is all kept or all moved -- and the moved runs are packed into d_scratch, slots 16-byte aligned;
 *                  pass 1 copies every moved run d_buf -> d_scratch, pass 2 d_scratch -> d_buf, both with k_raw_copy.  All reads come
 *                  before all writes, so any arrangement is safe: an asset shifted by fewer bytes than its length, two assets that swap
 *                  places, a store-fed chunk that lands on the old bytes of a moved one.  THE CARRY COMES FIRST: EINVAL once a blocks
 *                  call of the session has queued work (a scatter may have overwritten a source), and after it a blocks call whose d_out
 *                  is not d_buf is EINVAL.  cfg.verify: as carry, the feeding base chunks are hashed where they lie before pass 1; a
 *                  moved occurrence of a chunk that differs is left out of both passes and its destination keeps what the buffer held,
 *                  a kept one stays what it is, both count in base_chunks_mismatched and finish returns EBADF.  Without verify the base
 *                  is trusted.  EINVAL: no base; d_buf NULL while base-fed entries exist; d_scratch NULL or overlapping
 *                  [d_buf, d_buf + max(base_bytes, out_bytes)) while moved entries exist; more than 64 GiB would move (the slots are
 *                  placed by a 32-bit scan of 16-byte units).  ENOMEM: scratch_bytes below in_place_scratch_bound.  EEXIST: a carry of
 *                  either kind was called before.  A refused call queues and changes nothing.  A session in which everything is kept
 *                  accepts a NULL scratch and queues no copy.  Like carry it never waits, reads nothing back and allocates nothing
 *                  (scratch-pool growth and the BLAKE3 long-chunk exception apart); finish and the result are as for carry, and
 *                  occurrences_written / bytes_written include kept occurrences: they are in place and good.
 *   in_place_scratch_bound  host arithmetic over counters taken with the plan's one read-back: moved bytes + 16 x moved occurrences
 *                  + 64 (0 when nothing moves, and for a session without a base).
 *   in_place_stats  out[4] = {kept occurrences, kept bytes, moved occurrences, moved bytes}; all 0 for a session without a base. */
LTHIP_EXPORT int lthip_restore_layout_in_place(const void* base_version_index, size_t base_size, const uint64_t* base_offsets, uint64_t base_bytes,
                                               const void* target_version_index, size_t target_size, uint64_t align,
                                               uint64_t* target_offsets /*may be NULL*/, uint32_t* asset_count, uint64_t* total_bytes,
                                               uint32_t* kept_assets);
LTHIP_EXPORT size_t lthip_restore_in_place_scratch_bound(const lthip_restore* restore);
LTHIP_EXPORT int lthip_restore_in_place_stats(const lthip_restore* restore, uint64_t out[4]);
LTHIP_EXPORT int lthip_restore_carry_in_place(lthip_restore* restore, void* d_buf, void* d_scratch, uint64_t scratch_bytes);

/* ---- byte windows of assets: part of an asset, a rank's share (restore.hip, restore_windows.h) -----------------------------------------
 * The restore session at the granularity of the byte -- the device side of the reference's ranged read (BlockStoreStorageAPI_Read over
 * ReadFromBlock, lib/blockstorestorage/longtail_blockstorestorage.c:728 / :245): a part of a file out of a store, a restore divided
 * over ranks by the jobs the ingest is divided by, an asset or a version that does not fit one output buffer.
 *   create_windows  lthip_restore_create with windows[window_count] (host, read before the call returns) in place of asset_offsets.  A
 *                  window [offset, offset + length) of asset `asset` plans one occurrence per chunk of the asset from the one that holds
 *                  byte `offset` to the one that holds byte `offset + length - 1`, each CLIPPED to the window -- `skip` bytes into the
 *                  chunk, `clip` bytes long -- and written at dst + (its position inside the window).  The two chunks are found by
 *                  bisection over the asset's chunk prefix sums: a small window into an asset of 500 000 chunks does not walk them per
 *                  window.  Windows may name the same asset, and the same bytes, any number of times: each is its own occurrences.
 *                  Overlapping destinations are not checked (as asset offsets are not).  One window {a, 0, 0, size of a, offset of a}
 *                  per selected asset IS lthip_restore_create: the same output, needed_blocks and result -- that call and
 *                  lthip_restore_create_from_base are callers of the same routine.  It returns an ordinary lthip_restore:
 *                  needed_blocks, scratch_bound, blocks, finish, block_status and destroy work on it unchanged.
 *                    needed_blocks shrinks to the blocks that hold a chunk some window overlaps.
 *                    ENOENT only for a chunk some window overlaps that the StoreIndex does not hold (or holds with another size -- the
 *                           chunk's FULL size is compared, whatever the clip): a StoreIndex that lacks chunks no window touches is
 *                           accepted, so a rank may hold a partial StoreIndex.
 *                    EINVAL asset >= the version's asset count; reserved != 0; windows == NULL with window_count > 0; offset + length
 *                           beyond the asset's size; dst + length beyond out_bytes (both with overflow, and also for length 0); more
 *                           than 0x7FFFFFF0 occurrences in total (found before anything of that size is allocated).
 *                    Everything else is refused as lthip_restore_create refuses it; on any error nothing stays allocated and the
 *                    context stays usable.
 *                  A window of length 0 -- the only window a directory or an empty file admits -- plans nothing.
 *                  result.assets_selected: the distinct assets named by at least one window, whatever its length; occurrences,
 *                  occurrences_written and bytes_written count clipped occurrences and clipped bytes.
 *                  THE GUARANTEE is unchanged and per block: with verify every chunk of a delivered block is hashed WHOLE, also the
 *                  chunks a window uses a part of or not at all, so a block with a bad chunk outside every window still contributes
 *                  nothing; nothing is written outside [dst, dst + length) of any window.
 *                  A window session has no base: lthip_restore_carry and lthip_restore_carry_in_place return EINVAL on it.
 *   asset_sizes    host only.  sizes[asset count] (may be NULL), *asset_count and *target_chunk_size (may be NULL) of a serialized
 *                  VersionIndex: what lthip_job_count / lthip_make_jobs / lthip_partition_jobs want, for a caller that holds the
 *                  version as a blob.  EINVAL a NULL blob, EBADF as lthip_restore_layout.
 *   rank_windows   host arithmetic.  The share of `rank` as windows into a dense output buffer of that rank's own: its jobs of size > 0
 *                  in job order; a job that continues the one before it -- the same asset, its offset the end of that one -- joins its
 *                  window; a window's dst is the end of the window before it rounded up to `align` (a power of two, EINVAL otherwise;
 *                  the first window lies at 0); *out_bytes (may be NULL) = the end of the last window.  *window_count is always
 *                  filled; windows NULL or capacity below the count: the count (and *out_bytes) only, nothing is written -- ENOMEM
 *                  when windows were given.  Deterministic: every rank can compute every rank's table, which is what puts a file
 *                  together again from the ranks' buffers.
 * Out of scope: windows together with a base (create_from_base, carry, carry_in_place); decoding only the part of a tagged block that a
 * window needs -- a block is decoded whole, as the reference's ReadFromBlock does, so the cost follows the blocks needed.  What a
 * caller that reads in successive windows would decode twice stays decoded in a cache: "a cache of decoded blocks", below. */
typedef struct lthip_restore_window
{
    uint32_t asset;    /* index into the VersionIndex's assets */
    uint32_t reserved; /* 0 */
    uint64_t offset;   /* first byte of the asset that is wanted */
    uint64_t length;   /* 0: the window plans nothing */
    uint64_t dst;      /* where that byte goes in d_out */
} lthip_restore_window; /* 32 bytes */
#if defined(__cplusplus)
static_assert(sizeof(lthip_restore_window) == 32, "lthip_restore_window is 32 bytes");
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
_Static_assert(sizeof(lthip_restore_window) == 32, "lthip_restore_window is 32 bytes");
#endif
LTHIP_EXPORT int lthip_restore_create_windows(lthip_ctx* ctx, const lthip_restore_config* config, const void* version_index,
                                              size_t version_index_size, const void* store_index, size_t store_index_size,
                                              uint64_t window_count, const lthip_restore_window* windows /*host*/, uint64_t out_bytes,
                                              lthip_restore** out);
LTHIP_EXPORT int lthip_restore_asset_sizes(const void* version_index, size_t version_index_size, uint64_t* sizes /*may be NULL*/,
                                           uint32_t* asset_count, uint32_t* target_chunk_size);
LTHIP_EXPORT int lthip_restore_rank_windows(uint64_t job_count, const uint32_t* job_asset, const uint64_t* job_offset, const uint64_t* job_size,
                                            const uint32_t* job_rank, uint32_t rank, uint64_t align, lthip_restore_window* windows,
                                            uint64_t capacity, uint64_t* window_count, uint64_t* out_bytes);

/* ---- a cache of decoded blocks for the restore sessions (restore.hip, block_cache.h) ---------------------------------------------------
 * The device side of the reference's lib/lrublockstore, which it puts in front of its ranged reads: a set of decoded blocks in HBM that
 * outlives a session.  Good blocks delivered to a session with a cache stay resident; a later session on the same context finds its
 * needed blocks there, asks the caller only for the rest, and scatters the cached ones without fetching or decoding them again.  It
 * pays for successive windows (a boundary block is decoded once), for several passes over one version, and for images that live on
 * the host; it costs a copy per raw block and pays nothing for one full restore.  A session without a cache runs exactly as before.
 *   create         slot_count slots of slot_bytes rounded up to a multiple of 64, ONE device allocation of slot_count x that.  EINVAL: a
 *                  NULL context or out, 0 slots, 0 bytes.  ENOMEM: nothing stays allocated, the context stays usable.  A cache belongs
 *                  to one context (and its thread); it is destroyed after every session attached to it and before the context.
 *   entries        an entry is a block's chunks back to back (raw size bytes) at the start of a slot, keyed by (hash identifier, block
 *                  hash).  It keeps the block's chunk count, raw size, a 64-bit digest of its (chunk hash, chunk size) table as the
 *                  StoreIndex lists it (FNV-1a, block_cache.h), and whether the session that wrote it verified the chunks.  A block
 *                  whose raw size exceeds the slot size is never cached.  Replacement is strict LRU over the entries that no live
 *                  session reads (PINNED) and the slots no session is writing (RESERVED); an entry is USED by the set_cache that hit it
 *                  and by the finish that made it visible, numbered by one host counter.  All bookkeeping is host code.
 *   contains       host only.  held[i] = 1 when block_hashes[i] has a visible entry under hash_identifier.
 *   clear          every entry goes.  EBUSY, and nothing changes, while an entry is pinned or a slot is reserved.
 *   stats          out = {slots, slot bytes, resident entries, pinned entries, reserved slots, blocks hit, blocks inserted, entries
 *                  evicted, blocks bypassed, blocks dropped as bad} -- the last five summed since create.
 *   set_cache      once per session, after create and before the first blocks call; every kind of session takes it (whole assets,
 *                  windows, from a base, in place).  EEXIST: a second call.  EINVAL: NULL arguments, a cache of another context, or a
 *                  blocks call has queued work.  ENOMEM: the session's own small device tables; the session stays without a cache.
 *                  Every needed block is looked up: it is CACHE-FED when a visible entry has its key, chunk count, raw size and
 *                  digest -- and, for a verify session, was written by a verify session.  A verified entry is trusted as it lies and
 *                  is not hashed again, as the reference's LRU store trusts its blocks.  Cache-fed entries are pinned until finish
 *                  returns 0 or the session is destroyed.  needed_blocks, result.blocks_needed and scratch_bound shrink to the blocks
 *                  that are not cache-fed; a cache-fed block delivered anyway is accepted, counted as unneeded and not touched.
 *   from_cache     queues the scatter of every planned occurrence of the cache-fed blocks from their slots to d_out, on the context's
 *                  stream: it never waits, reads nothing back and is timed as LTHIP_K_GATHER.  Once per session (EEXIST), in any order
 *                  with blocks calls; EINVAL without a cache.  For an update in place it counts as a blocks call: after carry_in_place
 *                  d_out must be that buffer, and carry_in_place after it is EINVAL.  With no cache-fed block it queues nothing and
 *                  returns 0.  finish returns ENOENT while cache-fed blocks exist and from_cache has not been called (EBADF keeps
 *                  precedence); result.occurrences_written and bytes_written count the cache-fed occurrences once it was.
 *   blocks         with a cache, every needed block of the call reserves a slot when it fits one: the slot of its own entry when that
 *                  does not match (another StoreIndex, not verified) and is not pinned, else a free slot, else the least recently
 *                  used entry that is neither pinned nor reserved.  A tagged block is decoded INTO its slot instead of the scratch (no
 *                  copy; the decoders' capacity is the raw size, so nothing is written outside a slot).  A raw block's payload is
 *                  copied into its slot by k_restore_cache_copy behind the check, only when its status word is 0: no 4-byte word is
 *                  read that holds no byte of a chunk, and nothing of an image that is not exactly header + raw size.  A block that
 *                  gets no slot is BYPASSED and goes through the scratch as before; the output is the same either way.  The scratch
 *                  a call demands stays lthip_restore_scratch_bound, the worst case: a caller never predicts what the cache takes.
 *   finish         a reserved slot is invisible.  finish, which reads the status words anyway, COMMITS every reserved block whose
 *                  status is 0 -- it becomes visible, verified = the session's verify setting -- and releases every other one.  When
 *                  two sessions reserved the same block, the later commit replaces the earlier entry, or is dropped when that entry
 *                  is pinned.  Destroying a session that did not finish releases its reservations and pins.
 *   cache_stats    out = {cache-fed blocks, their raw bytes, blocks inserted, blocks bypassed (too large, or no slot to be had), inserted
 *                  blocks dropped as bad, cache-fed entries scattered}.
 * THE GUARANTEE extended: no byte of a bad block is ever served from the cache, and a session with a cache writes nothing outside the
 * selected windows.  What verify-off trusts, the cache trusts for verify-off sessions: a raw block with a right header and a wrong chunk
 * byte is served as delivered -- to sessions that do not verify, never to one that does. */
typedef struct lthip_block_cache lthip_block_cache;
LTHIP_EXPORT int lthip_block_cache_create(lthip_ctx* ctx, uint32_t slot_count, uint64_t slot_bytes, lthip_block_cache** out);
LTHIP_EXPORT void lthip_block_cache_destroy(lthip_block_cache* cache);
LTHIP_EXPORT int lthip_block_cache_contains(const lthip_block_cache* cache, uint32_t hash_identifier, uint32_t count,
                                            const uint64_t* block_hashes /*host*/, uint8_t* held /*host*/);
LTHIP_EXPORT int lthip_block_cache_clear(lthip_block_cache* cache);
LTHIP_EXPORT int lthip_block_cache_stats(const lthip_block_cache* cache, uint64_t out[10]);
LTHIP_EXPORT int lthip_restore_set_cache(lthip_restore* restore, lthip_block_cache* cache);
LTHIP_EXPORT int lthip_restore_from_cache(lthip_restore* restore, void* d_out);
LTHIP_EXPORT int lthip_restore_cache_stats(const lthip_restore* restore, uint64_t out[6]);

/* ---- one-file archives: pack ingested blocks, restore from an archive (archive.hip, archive_layout.h, restore.hip) ---------------------
 * The device side of lib/archiveblockstore: the single file golongtail's pack / unpack move around, [ArchiveIndex][block][block]...
 * (Longtail_CreateArchiveIndex / Longtail_ReadArchiveIndex, src/longtail.c:9921-10090).  The index is
 *   u32 version (LONGTAIL_VERSION(0,0,1))   u32 index_data_size (of the whole index)   the serialized StoreIndex
 *   u64 block_start_offsets[nb], relative to the END of the index   u32 block_sizes[nb]   the serialized VersionIndex   pad to 8
 * byte for byte as the reference writes it (its pad bytes are uninitialised, ours are zero; the u64 table is only 4-byte aligned when
 * nb + m is odd, every word goes through memcpy).  The BODY behind it holds the stored-block images back to back, in any order and at
 * ANY byte position.  File I/O is the caller's: these calls see the index in host memory and pieces of the body in HBM.
 * THE INDEX, host only, no context:
 *   index_size     the bytes of the index of these two blobs, (8 + S + 12 nb + V + 7) & ~7.  EBADF: a blob lthip_restore_layout / create
 *                  would call malformed; EINVAL: the index would not fit the 32 bits of index_data_size (nothing is truncated).
 *   write_index    the index with block b at body offset block_offsets[b], block_sizes[b] bytes long, into out[0, capacity); ENOMEM below
 *                  index_size (nothing written).
 *   peek           the first eight bytes of a file -> *index_bytes, so that a reader knows how much to read.  EBADF: another version.
 *   open           deep-copies the index (it may be freed on return).  body_bytes: the size of the body (file size - index_bytes), or
 *                  UINT64_MAX when it is not known -- lthip_archive_body_bytes is then the end of the last block.  EBADF: index_bytes is
 *                  not the stored size (a short or over-long index); another version; counts that leave the index; a block whose
 *                  offset + size leaves body_bytes; a block smaller than its own header (20 + 12 n, + 8 when tagged); a malformed
 *                  StoreIndex or VersionIndex.  Blocks may lie in any order (the reference writes them as its workers complete) and may
 *                  overlap: every image is checked against the StoreIndex when it is delivered.
 *   store_index / version_index / block_count / block_offsets / block_sizes / body_bytes   views into the handle, valid until close.  A
 *                  serialized VersionIndex does not store the length of its name data: as Longtail_ReadArchiveIndex does, the
 *                  VersionIndex blob is the REST of the index, up to 7 pad bytes included; lthip_restore_* accept it as it is.
 * THE WRITER:
 *   append         takes `count` images exactly as lthip_ingest_stream_images / lthip_ingest_images hand them out (image i at d_arena +
 *                  image_offsets[i], image_sizes[i] bytes; host tables, free on return) and queues ONE kernel, k_archive_pack (grid: images
 *                  x 256 KiB pieces, the copy is lthip_wg_copy), that lays them densely from d_dst[0]: *bytes_written = the sum of the
 *                  sizes, nothing is written at or beyond d_dst + *bytes_written, no 4-byte word is read that holds no byte of an image.
 *                  The archive's body is the concatenation of all calls' outputs: the writer carries the cursor and records every
 *                  block's offset and size; the caller drains d_dst (to the host, to a file) between calls.  ENOMEM before any work when
 *                  the call's images exceed dst_capacity.  Never waits for the device (but where the context's table pool has to grow).
 *                  Timed as LTHIP_K_GATHER.
 *   blocks         the tables recorded so far (the writer's, valid until its next call) and the body's size.
 *   finish         writes the index from the recorded tables.  EINVAL: the appended blocks are not the StoreIndex's block count, or an
 *                  appended size is below that block's header size.  ENOMEM with *index_bytes filled in when h_index is NULL or the
 *                  capacity is short: call again.  Does not wait for the device either.
 * THE READER: the restore session fed from pieces of the body.
 *   archive_blocks delivers every needed, not yet delivered block that lies WHOLLY inside body bytes [window_first_byte, +window_bytes),
 *                  which lie at d_window, at whatever byte position it has there: lthip_restore_blocks without the alignment rule.
 *                  Unneeded blocks are not touched, and neither are blocks of the archive the session's StoreIndex does not hold.
 *                  *delivered = the blocks this call delivered; *next_byte = the lowest body offset of a needed block still outstanding,
 *                  or lthip_archive_body_bytes when there is none: a reader that streams the file in pieces starts its next read there.
 *                  A window that holds no complete needed block returns 0 with *delivered == 0.  The refusals (ENOTSUP, ENOMEM for a
 *                  scratch below archive_scratch_bound, EINVAL for a null scratch or output), the queued stages and THE GUARANTEE are
 *                  those of lthip_restore_blocks; a refused call delivers nothing and leaves the session usable.  The check is a second
 *                  kernel, k_restore_check_images_any, that assembles every header dword from the two aligned dwords around it: no dword is
 *                  read that holds no byte of the image, an image may end at the last byte of the allocation.  Decoders, verify, scatter
 *                  and the cache copy take any byte position as they are.  Works with verify, with a base, with window sessions and with
 *                  an attached cache.
 *   archive_scratch_bound   host arithmetic: the scratch an archive_blocks call with this window needs now.
 *   archive_ranges host only.  The body ranges {first byte, bytes} of the needed, outstanding blocks, sorted, merged where the gap between
 *                  two is at most max_gap: ranges[2 i], ranges[2 i + 1].  ranges NULL or capacity (in ranges) too small: the count only. */
typedef struct lthip_archive lthip_archive;
typedef struct lthip_archive_writer lthip_archive_writer;
LTHIP_EXPORT int lthip_archive_index_size(const void* store_index, size_t store_index_size, const void* version_index, size_t version_index_size,
                                          uint64_t* out_bytes);
LTHIP_EXPORT int lthip_archive_write_index(const void* store_index, size_t store_index_size, const void* version_index, size_t version_index_size,
                                           const uint64_t* block_offsets /*host, [nb]*/, const uint32_t* block_sizes /*host, [nb]*/, void* out,
                                           size_t capacity);
LTHIP_EXPORT int lthip_archive_peek(const void* first_8_bytes, uint64_t* index_bytes);
LTHIP_EXPORT int lthip_archive_open(const void* index, size_t index_bytes, uint64_t body_bytes /* UINT64_MAX: unknown */, lthip_archive** out);
LTHIP_EXPORT void lthip_archive_close(lthip_archive* archive);
LTHIP_EXPORT const void* lthip_archive_store_index(const lthip_archive* archive, size_t* size);
LTHIP_EXPORT const void* lthip_archive_version_index(const lthip_archive* archive, size_t* size);
LTHIP_EXPORT uint32_t lthip_archive_block_count(const lthip_archive* archive);
LTHIP_EXPORT const uint64_t* lthip_archive_block_offsets(const lthip_archive* archive);
LTHIP_EXPORT const uint32_t* lthip_archive_block_sizes(const lthip_archive* archive);
LTHIP_EXPORT uint64_t lthip_archive_body_bytes(const lthip_archive* archive);
LTHIP_EXPORT int lthip_archive_writer_create(lthip_ctx* ctx, lthip_archive_writer** out);
LTHIP_EXPORT void lthip_archive_writer_destroy(lthip_archive_writer* writer);
LTHIP_EXPORT int lthip_archive_writer_append(lthip_archive_writer* writer, const void* d_arena, uint32_t count,
                                             const uint64_t* image_offsets /*host*/, const uint32_t* image_sizes /*host*/, void* d_dst,
                                             uint64_t dst_capacity, uint64_t* bytes_written);
LTHIP_EXPORT int lthip_archive_writer_blocks(const lthip_archive_writer* writer, uint64_t* block_count, const uint64_t** offsets,
                                             const uint32_t** sizes, uint64_t* body_bytes);
LTHIP_EXPORT int lthip_archive_writer_finish(lthip_archive_writer* writer, const void* store_index, size_t store_index_size,
                                             const void* version_index, size_t version_index_size, void* h_index, size_t capacity,
                                             uint64_t* index_bytes);
LTHIP_EXPORT int lthip_restore_archive_blocks(lthip_restore* restore, const lthip_archive* archive, const void* d_window,
                                              uint64_t window_first_byte, uint64_t window_bytes, void* d_scratch, uint64_t scratch_bytes,
                                              void* d_out, uint32_t* delivered, uint64_t* next_byte);
LTHIP_EXPORT size_t lthip_restore_archive_scratch_bound(const lthip_restore* restore, const lthip_archive* archive, uint64_t window_first_byte,
                                                        uint64_t window_bytes);
LTHIP_EXPORT int lthip_restore_archive_ranges(const lthip_restore* restore, const lthip_archive* archive, uint64_t max_gap,
                                              uint64_t* ranges /*host, [2 * capacity]*/, uint64_t capacity, uint64_t* count);

/* ---- store index operations: prune, merge, a version's chunk hashes (store_index_ops.h) -------------------------------------------------
 * Host only, no context: what keeps a store's index in step with its blocks.  The StoreIndexes the ingest sessions return are small and
 * many -- one per slice of a host-fed loop, one per rank, one per incremental ingest; merge folds them into the store's index, prune
 * takes the blocks a caller deleted out of it.  The outputs are serialized StoreIndexes, byte for byte the reference's:
 *   prune   Longtail_PruneStoreIndex (src/longtail.c:9287) + Longtail_WriteStoreIndexToBuffer: the blocks of store_index whose hash is
 *           among keep_block_hashes[0, keep_count), in store_index's order.  Repeats and unknown hashes in the keep list change nothing;
 *           a block hash that stands twice in store_index is kept twice; the hash identifier is store_index's even when nothing is kept.
 *   merge   Longtail_MergeStoreIndex (:9151) + Longtail_WriteStoreIndexToBuffer: local's blocks in their order, then remote's blocks
 *           that local does not hold.  A block hash is taken once, its first occurrence gives the tag and the chunk list (a block both
 *           sides hold is local's).  The hash identifier is local's when local has blocks, else remote's when remote has blocks, else 0.
 *   version_chunk_hashes   the chunk hashes of a serialized VersionIndex, in its order: *count of them into out[0, capacity).  out NULL:
 *           the count only.  The live set of the versions a caller keeps is the concatenation (lthip_get_existing_store_index and the
 *           store sets take duplicates).
 * Refusals.  EINVAL: a null blob or size pointer, keep_count without a list; merge: BOTH indexes have blocks and their hash identifiers
 * differ; a result whose block or chunk count leaves 32 bits.  EBADF: a blob lthip_restore_create would call malformed (short, another
 * version, a block whose chunks leave the chunk list).  ENOMEM with *out_size (*count) set: out is NULL or out_capacity too small --
 * nothing is written, call again.  Blobs and `out` may lie at any alignment; the keep list and the hash output are the caller's uint64
 * arrays.  Input and output must not overlap.
 * These calls do not touch a block. */
LTHIP_EXPORT int lthip_store_index_prune(const void* store_index, size_t store_index_size, uint32_t keep_count,
                                         const uint64_t* keep_block_hashes /*host*/, void* out, size_t out_capacity, size_t* out_size);
LTHIP_EXPORT int lthip_store_index_merge(const void* local, size_t local_size, const void* remote, size_t remote_size, void* out,
                                         size_t out_capacity, size_t* out_size);
LTHIP_EXPORT int lthip_version_chunk_hashes(const void* version_index, size_t version_index_size, uint64_t* out /*host, may be NULL*/,
                                            uint64_t capacity, uint64_t* count);

/* ---- the repack session: the live chunks of under-used blocks into new blocks (repack.hip, repack_plan.h) -----------------------------
 * Acting on min_block_usage_percent.  A store that has seen many versions fills with blocks of which a fifth is still wanted; this
 * session takes the store's StoreIndex, the LIVE set (a device array of chunk hashes, typically the concatenated
 * lthip_version_chunk_hashes of the versions that are kept; duplicates allowed) and a threshold, decides which blocks stay, rewrites the
 * live chunks of the others into new stored-block images on the device, from the blocks themselves, and returns the indexes that
 * describe the store afterwards.  No file is read, no chunk is cut or hashed again but to verify.  With `live` = the distinct hashes of
 * the live list in first-occurrence order:
 *   kept     exactly the blocks of lthip_get_existing_store_index(store_index, live list, min_block_usage_percent), and
 *            lthip_repack_kept_index is byte for byte that call's output.  A block below the threshold, a block with no live chunk and a
 *            block whose live chunks an earlier block of that call's walk already holds are all not kept.
 *   moved    the hashes of `live` that no kept block holds, in live's order.  A moved chunk's size is the StoreIndex's, its tag the tag
 *            of its SOURCE block: the first block in StoreIndex order that holds it.  A chunk two non-kept blocks hold is moved once,
 *            from the first; a chunk a kept block also holds is not moved.
 *   source   the blocks that are the source of at least one moved chunk, in StoreIndex order.  Only these have to be delivered.
 *   dropped  every block that is not kept, in StoreIndex order.
 *   new      byte for byte lthip_create_missing_content(existing = the kept blocks' chunk hashes, chunks = live with the sizes and tags
 *            above, the StoreIndex's hash identifier, cfg.max_block_size, cfg.max_chunks_per_block) -- also when nothing is missing.
 *   after    lthip_repack_store_index: lthip_store_index_merge(local = kept, remote = new), with ONE correction.  The reference takes a
 *            found block's tag from m_BlockTags[first chunk index] (src/longtail.c:7307) and lthip_get_existing_store_index mirrors it;
 *            in a store of mixed tags that word is not the block's tag, and no restore session accepts an image against it.  The
 *            index handed out here carries every kept block's OWN tag, as the store's index records it; where the two agree it is
 *            the plain merge of lthip_repack_kept_index and the new index.
 * THE SAFETY CONTRACT: delete dropped blocks only after lthip_repack_finish returned 0 and the new images are stored.
 *   create       builds the whole plan; the stream is waited for here and nowhere else before finish (the two index calls wait as they
 *                always do, the plan reads back once, the restore plan once).  EINVAL: cfg NULL, a struct_size that does not reach
 *                max_chunks_per_block, a percent above 100, a zero max_block_size or max_chunks_per_block.  EBADF: a malformed index.
 *                ENOENT: the live list names a hash the StoreIndex does not hold.  ENOTSUP: a SOURCE block's tag is not 0, 'lz42' or
 *                'ztd1'..'ztd5' (such a tag on a kept block, or on a dropped block that is no source, is fine).  On any error nothing
 *                stays allocated and the context stays usable.
 *   plan_info    what the plan came to (struct_size honoured); host only, as are the three block lists (hashes NULL or capacity too
 *                small: the count alone) and lthip_repack_kept_index (ENOMEM with *size set: out NULL or too small).
 *   the work buffer   ONE caller buffer of info.work_bytes (device memory, 8-byte aligned), laid out by the session: a staging region
 *                of info.staging_bytes, then the images at 8-byte aligned offsets, each with room for
 *                lthip_stored_block_header_size(n) + the codec's bound, or lthip_block_index_size(n) + raw size for tag 0.  A tagged
 *                new block's chunks are staged back to back in the new index's chunk order: its raw payload is one byte range the
 *                codec reads where it lies.  A tag-0 new block's chunks are scattered straight to their final positions inside its
 *                image and never pass through staging.
 *   scratch_bound, blocks, block_status   lthip_restore_scratch_bound / _blocks / _block_status over the source blocks, d_work in the
 *                place of d_out, with every refusal and property of those calls: ENOENT unknown hash, EEXIST delivered before or twice,
 *                EINVAL misaligned offset, ENOMEM scratch below the bound; a block that is no source is accepted, counted and not
 *                touched; nothing is waited for; sources may come in any number of calls, in any order; scratch and images may be
 *                reused once a call's work has run.  THE GUARANTEE of the restore session holds: no byte of a bad block reaches d_work.
 *                With cfg.verify every chunk of a delivered source block is hashed and compared.  Every call names the same d_work;
 *                EINVAL, the session unchanged, for another one or one that is not 8-byte aligned (write refuses the same).
 *   write        queues the block writer of the ingest sessions for all new blocks: the codec by tag from staging into the images,
 *                BlockIndex and [raw][compressed] words; the block hashes are the new index's.  ENOENT, nothing queued, while source
 *                blocks are outstanding: deliver and call again.  EEXIST on a second successful call.  ENOMEM: work_bytes below
 *                info.work_bytes.
 *   finish       the session's one full synchronisation.  0 only if every source block was delivered and good and the images were
 *                written; then the new index goes to h_new_index (NULL: *size alone; ENOMEM when capacity is too small -- call again).
 *                ENOENT: source blocks, or write, are outstanding.  EBADF: a delivered block was bad -- it takes precedence; NO IMAGE
 *                TABLE IS HANDED OUT, lthip_repack_images and lthip_repack_store_index return EBADF from then on, the caller must
 *                delete nothing and the session is over.  The result is filled either way (struct_size honoured).
 *   images       host tables, valid after finish returned 0 and until destroy: image i of the new index lies at d_work + offsets[i]
 *                and is sizes[i] bytes long.
 * Re-tagging moved chunks, a repack whose moved bytes do not fit one work buffer, and every file operation are not part of it.  One
 * session belongs to one context (and its thread) and must be destroyed before it. */
typedef struct lthip_repack lthip_repack;
typedef struct lthip_repack_config
{
    uint64_t struct_size;             /* IN: sizeof(lthip_repack_config) of the caller's header; the library reads at most that */
    uint32_t min_block_usage_percent; /* 0 .. 100; 0 keeps every block that holds a live chunk no earlier block of the walk holds */
    uint32_t max_block_size;          /* of the new blocks, as lthip_create_missing_content takes them */
    uint32_t max_chunks_per_block;
    uint32_t verify;                  /* 0 or 1 */
} lthip_repack_config;
typedef struct lthip_repack_info
{
    uint64_t struct_size; /* IN: sizeof(lthip_repack_info) of the caller's header; the library fills at most that */
    uint64_t blocks_total, blocks_kept, blocks_dropped, blocks_source;
    uint64_t live_chunks /* distinct */, moved_chunks, moved_bytes;
    uint64_t new_blocks;
    uint64_t staging_bytes, work_bytes;
    uint64_t kept_index_size, new_index_size, store_index_size;
} lthip_repack_info;
typedef struct lthip_repack_result
{
    uint64_t struct_size; /* IN: sizeof(lthip_repack_result) of the caller's header; the library fills at most that */
    uint64_t blocks_source, blocks_delivered /* all accepted blocks */, blocks_bad;
    uint64_t chunks_mismatched;                           /* verify: chunks whose hash differed */
    uint64_t raw_bytes_written, compressed_bytes_written; /* of the new blocks: chunk bytes, payload bytes (0 unless finish returned 0) */
    uint64_t decoded_bytes;                               /* raw bytes of the tagged source blocks whose decoder returned the raw size */
} lthip_repack_result;
LTHIP_EXPORT int lthip_repack_create(lthip_ctx* ctx, const lthip_repack_config* config, const void* store_index, size_t store_index_size,
                                     uint64_t live_count, const uint64_t* d_live_hashes, lthip_repack** out);
LTHIP_EXPORT void lthip_repack_destroy(lthip_repack* repack);
LTHIP_EXPORT int lthip_repack_plan_info(const lthip_repack* repack, lthip_repack_info* out_info);
LTHIP_EXPORT int lthip_repack_kept_blocks(const lthip_repack* repack, uint64_t* block_hashes, uint64_t capacity, uint64_t* count);
LTHIP_EXPORT int lthip_repack_dropped_blocks(const lthip_repack* repack, uint64_t* block_hashes, uint64_t capacity, uint64_t* count);
LTHIP_EXPORT int lthip_repack_source_blocks(const lthip_repack* repack, uint64_t* block_hashes, uint64_t capacity, uint64_t* count);
LTHIP_EXPORT int lthip_repack_kept_index(const lthip_repack* repack, void* out, size_t capacity, size_t* size);
LTHIP_EXPORT size_t lthip_repack_scratch_bound(const lthip_repack* repack, uint32_t block_count, const uint64_t* block_hashes);
LTHIP_EXPORT int lthip_repack_blocks(lthip_repack* repack, uint32_t block_count, const uint64_t* block_hashes /*host*/, const void* d_images,
                                     const uint64_t* image_offsets /*host, 8-byte aligned*/, const uint32_t* image_sizes /*host*/,
                                     void* d_scratch, uint64_t scratch_bytes, void* d_work);
LTHIP_EXPORT int lthip_repack_write(lthip_repack* repack, void* d_work, uint64_t work_bytes);
LTHIP_EXPORT int lthip_repack_finish(lthip_repack* repack, void* h_new_index, size_t capacity, size_t* size, lthip_repack_result* out_result);
LTHIP_EXPORT int lthip_repack_images(const lthip_repack* repack, uint64_t* count, const uint64_t** offsets, const uint32_t** sizes);
LTHIP_EXPORT int lthip_repack_store_index(const lthip_repack* repack, void* out, size_t capacity, size_t* size);
LTHIP_EXPORT int lthip_repack_block_status(const lthip_repack* repack, uint32_t count, const uint64_t* block_hashes, uint32_t* status);

/* ---- multi-GPU work division, host functions -----------------------------------------------------------
 * The unit of independence is the reference's own job: one (asset, target_chunk_size*1024-byte part) of ChunkAssets
 * (src/longtail.c:2396-2458).  lthip_job_count / lthip_make_jobs list the jobs of a tree exactly as :2399-2404 / :2432-2457 do
 * (asset order, 1 + size / part jobs per asset: an exact multiple ends with an empty job, a directory is one empty job).
 * lthip_partition_jobs assigns them to ranks -- deterministic, so every rank computes the same table without communication:
 *   LTHIP_PARTITION_RANGE  contiguous job ranges with equal byte shares (rank-major order == job order; an asset's parts may
 *                          straddle ranks: intra-file segment sharding, BASELINE.json configs[4])
 *   LTHIP_PARTITION_LPT    longest processing time first: jobs by size descending, each to the least loaded rank
 *   LTHIP_PARTITION_MOD    job index mod rank_count (uniform trees)
 * rank_bytes[r] (may be NULL) receives the bytes assigned to rank r. */
enum lthip_partition_policy
{
    LTHIP_PARTITION_RANGE = 0,
    LTHIP_PARTITION_LPT = 1,
    LTHIP_PARTITION_MOD = 2
};
LTHIP_EXPORT uint64_t lthip_job_count(uint32_t asset_count, const uint64_t* asset_sizes, uint32_t target_chunk_size);
LTHIP_EXPORT int lthip_make_jobs(uint32_t asset_count, const uint64_t* asset_sizes, uint32_t target_chunk_size, uint64_t capacity,
                                 uint32_t* job_asset, uint64_t* job_offset /* within the asset */, uint64_t* job_size);
LTHIP_EXPORT int lthip_partition_jobs(uint64_t job_count, const uint64_t* job_sizes, uint32_t rank_count, int policy,
                                      uint32_t* job_rank, uint64_t* rank_bytes);
/* The exchange: every rank chunks + hashes its jobs in ascending job order, then the ranks all-gather (1) their per-job chunk
 * counts, padded to count_stride entries per rank, and (2) their chunk hash / length arrays, padded to chunk_stride entries per
 * rank.  This function says where job j's run of chunks sits in the gathered arrays (job_src[j], element index) and where it
 * belongs in job order (job_dst[j]; job_dst[job_count] = total chunks) -- the order ChunkAssets concatenates in (:2499-2517),
 * which the serial first-seen pass (:2951-2970) depends on.  One lthip_gather_ranges per array applies it.  EINVAL when the
 * counts disagree with the assignment. */
LTHIP_EXPORT int lthip_exchange_layout(uint64_t job_count, const uint32_t* job_rank, uint32_t rank_count,
                                       const uint32_t* gathered_counts, uint64_t count_stride, uint64_t chunk_stride,
                                       uint64_t* job_src, uint64_t* job_dst /* job_count + 1 */, uint32_t* job_chunks /* may be NULL */);
/* The layout as the device reorder wants it: runs of jobs that are contiguous on both sides merged (range policy: one run per rank),
 * then cut into pieces of at most max_piece elements (a workgroup per piece).  Returns the number of pieces; out arrays NULL or
 * capacity too small: count only.  Host function, O(jobs). */
LTHIP_EXPORT uint64_t lthip_exchange_ranges(uint64_t job_count, const uint64_t* job_src, const uint64_t* job_dst,
                                            const uint32_t* job_chunks, uint64_t max_piece, uint64_t capacity, uint64_t* out_src,
                                            uint64_t* out_dst, uint32_t* out_cnt);
/* Applies it on the device: d_out[range_dst[i] ..) = d_gathered[range_src[i] .. + range_cnt[i]) in elements of elem_bytes (host
 * tables, staged through the context's pinned ring; asynchronous on the context's stream).  Every array of the exchange -- hashes,
 * lengths, the first-seen answers -- goes through the same tables. */
LTHIP_EXPORT int lthip_exchange_reorder(lthip_ctx* ctx, const void* d_gathered, void* d_out, uint32_t elem_bytes,
                                        uint64_t range_count, const uint64_t* range_src, const uint64_t* range_dst,
                                        const uint32_t* range_cnt);
/* Positions of this rank's chunks in job order (what the sharded first-seen table is keyed with): d_out[k] = global_first[m] +
 * (k - local_first[m]) for the own job m that holds local chunk k; local_first / global_first: host arrays of my_job_count entries,
 * index of each own job's first chunk in the rank's own lists / in the tree's job-ordered lists. */
LTHIP_EXPORT int lthip_job_ordinals(lthip_ctx* ctx, uint64_t my_job_count, const uint32_t* local_first, const uint32_t* global_first,
                                    uint64_t local_chunks, uint32_t* d_out);

/* The collective itself behind the C ABI (comm.hip): RCCL's all-gather on the context's stream, one process per GPU.  RCCL is
 * bound at run time (dlopen): ENOSYS where it is missing.  Rank 0 makes the 128-byte id, the embedder carries it to the other
 * processes (any side channel), every rank creates its communicator with it.  lthip_comm_allgather: every rank contributes
 * `count` elements of `elem_bytes` from d_send; d_recv receives rank r's contribution at element r * count (the padded
 * all-gathers lthip_exchange_layout describes).  Asynchronous on the context's stream like every other bulk call.
 *
 * lthip_comm_alltoallv: the exchange of the SHARDED first-seen table (the serial pass of src/longtail.c:2951-2970 restated as "minimum
 * position per hash", the table split by hash over the ranks): rank r sends send_counts[p] elements starting at element
 * send_displs[p] of d_send to every rank p and receives recv_counts[p] elements from it at element recv_displs[p] of d_recv
 * (host arrays of nranks entries; recv_counts[p] must equal rank p's send_counts[r] -- the ranks learn them by an all-gather of
 * their send counts).  RCCL: one group of ncclSend / ncclRecv pairs on the context's stream -- point to point, the natural shape on
 * xGMI.  lthip_comm_info: the communicator's size AS THE TRANSPORT REPORTS IT (ncclCommCount), this process's rank, the transport.
 *
 * Transports.  LTHIP_COMM_RCCL is the product path.  LTHIP_COMM_SHM is a stand-in for boxes without N GPUs: lthip_comm_unique_id
 * makes a shared-memory id when LTHIP_COMM_TRANSPORT=shm is set in the environment of the process that makes the id, and every
 * lthip_comm_create that receives such an id attaches to the segment /dev/shm/lthip_comm_<id>; the same entry points then move the
 * bytes through host memory, synchronously (with ctx == NULL the pointers are host pointers: the CPU tests).  It exists so that the
 * torch-free launch, the id hand-over and the exchange can be exercised with N processes on one GPU; it is never a measured path. */
#define LTHIP_COMM_ID_BYTES 128
#define LTHIP_COMM_RCCL 1
#define LTHIP_COMM_SHM 2
typedef struct lthip_comm lthip_comm;
LTHIP_EXPORT int lthip_comm_unique_id(void* id128);
LTHIP_EXPORT int lthip_comm_create(lthip_ctx* ctx, int nranks, int rank, const void* id128, lthip_comm** out);
LTHIP_EXPORT int lthip_comm_destroy(lthip_comm* comm);
/* The file RCCL was bound from -- $LTHIP_RCCL_PATH, else a librccl already mapped into the process (torch's), else librccl.so.1 /
 * librccl.so on the loader's path and in /opt/rocm/lib, else beside a mapped libtorch -- or, when none was found, what was tried;
 * *out_how (may be NULL) names the rule.  Loads the library on first use. */
LTHIP_EXPORT const char* lthip_comm_library(const char** out_how);
LTHIP_EXPORT int lthip_comm_info(const lthip_comm* comm, int* out_nranks, int* out_rank, int* out_transport);
LTHIP_EXPORT int lthip_comm_allgather(lthip_ctx* ctx, lthip_comm* comm, const void* d_send, void* d_recv, uint64_t count,
                                      uint32_t elem_bytes);
LTHIP_EXPORT int lthip_comm_alltoallv(lthip_ctx* ctx, lthip_comm* comm, const void* d_send, const uint64_t* send_counts /*host*/,
                                      const uint64_t* send_displs /*host*/, void* d_recv, const uint64_t* recv_counts /*host*/,
                                      const uint64_t* recv_displs /*host*/, uint32_t elem_bytes);

/* ---- synthetic assets (include/longtail_synth.h), bench/test input generator ------------------------ */
LTHIP_EXPORT int lthip_synth_fill(lthip_ctx* ctx, void* d_dst, uint32_t asset_count, const uint64_t* asset_offsets /*host*/,
                                  const uint64_t* asset_sizes /*host*/, const uint64_t* asset_seeds /*host*/, int kind);
/* the same for RANGES of assets: range i = bytes [asset_skips[i], asset_skips[i] + asset_sizes[i]) of the asset with seed
 * asset_seeds[i] (skips are multiples of 16) -- a rank generates only the parts of a large asset it owns */
LTHIP_EXPORT int lthip_synth_fill_ranges(lthip_ctx* ctx, void* d_dst, uint32_t asset_count, const uint64_t* asset_offsets /*host*/,
                                         const uint64_t* asset_sizes /*host*/, const uint64_t* asset_seeds /*host*/,
                                         const uint64_t* asset_skips /*host, may be NULL*/, int kind);

#ifdef __cplusplus
}
#endif
#endif
