/* plugin_blake2.c -- Longtail_HashAPI 'blk2' (BLAKE2s, 64-bit) on the GPU: the object of plugin_hash.c over the lthip_blake2s_* calls.
 *
 * Mirrors lib/blake2/longtail_blake2.c of the reference: Longtail_CreateHipBlake2HashAPI <-> Longtail_CreateBlake2HashAPI,
 * GetIdentifier -> 'blk2' 0x626c6b32, BeginContext / Hash / EndContext / HashBuffer as the BLAKE3 object's.
 *
 * Paired with the HIP chunker.  A published window carries BLAKE3 digests.  Its BLAKE2 table is filled lazily: the first HashBuffer of
 * one of its chunks hashes ALL of the window's chunks with one lthip_blake2s_ranges call -- from the window's device copy when the
 * chunker left it resident (the direct path), else uploaded again from the pinned window (the batcher chunks small windows in an arena
 * of its own) -- and every later HashBuffer of the window is a table read.  Only the calling thread's current window is consulted
 * (longtail's DynamicChunking calls NextChunk and HashBuffer alternately on one thread, src/longtail.c:2231-2296): the registry keeps
 * it stable meanwhile, and no other thread reads or fills the table.  Anything else is hashed on the GPU by itself.
 */
#include "plugin_common.h"

#define LONGTAIL_HIP_BLAKE2_ID ((((uint32_t)'b') << 24) + (((uint32_t)'l') << 16) + (((uint32_t)'k') << 8) + ((uint32_t)'2'))

/* plugin_hash.c collects stream batches of LTHIP_B3_STREAM_BATCH bytes for every kind */
#if LTHIP_B3_STREAM_BATCH != LTHIP_B2S_STREAM_BATCH
#error "the BLAKE3 and BLAKE2s stream batches differ"
#endif

static int b2_window_digest(const struct ltp_window* pub, uint32_t index, void* arg)
{
    struct ltp_chunk_window* w = pub->owner;
    if (!w->b2_ready)
    {
        lthip_ctx* ctx = ltp_thread_ctx();
        if (!ctx)
            return -ENODEV;
        int err = 0;
        if (!w->h_hash2)
            err = lthip_malloc_pinned(ctx, (size_t)w->ccap * 8, (void**)&w->h_hash2);
        if (!err && !w->d_resident)
        {
            err = lthip_copy_h2d(ctx, w->d_win, pub->base, (size_t)pub->size);
            if (!err) err = lthip_copy_h2d(ctx, w->d_off, pub->offsets, (size_t)pub->count * 8);
            if (!err) err = lthip_copy_h2d(ctx, w->d_len, pub->lens, (size_t)pub->count * 4);
        }
        if (!err) err = lthip_blake2s_ranges(ctx, w->d_win, pub->count, w->d_off, w->d_len, w->max_chunk, w->d_hash);
        if (!err) err = lthip_copy_d2h(ctx, w->h_hash2, w->d_hash, (size_t)pub->count * 8);
        if (!err) err = lthip_ctx_sync(ctx);
        if (err)
            return -err;
        w->b2_ready = 1;
    }
    *(uint64_t*)arg = w->h_hash2[index];
    return 1;
}

static int b2_window_lookup(const void* data, uint32_t len, uint64_t* out_hash)
{
    const int r = ltp_window_with_current(data, len, b2_window_digest, out_hash);
    return r < 0 && r != -1 ? r : (r == 1);
}

static const struct ltp_hash_kind g_blake2 = {LONGTAIL_HIP_BLAKE2_ID, lthip_blake2s_one, lthip_blake2s_ranges, lthip_b2s_stream_batch,
                                              lthip_b2s_stream_final, LTHIP_B2S_STREAM_STATE_BYTES, 0, b2_window_lookup};

struct Longtail_HashAPI* Longtail_CreateHipBlake2HashAPI(void) { return ltp_create_hash_api(&g_blake2); }
