/* plugin_hash.c -- Longtail_HashAPI (BLAKE3 and BLAKE2s, 64-bit) on the GPU; C99 host code over the lthip_* C ABI.
 *
 * Mirrors lib/blake3/longtail_blake3.c of the reference:
 *   Longtail_CreateHipBlake3HashAPI <-> Longtail_CreateBlake3HashAPI (:124-141)
 *   GetIdentifier                   <-> Blake3Hash_GetIdentifier     (:15-22)   -> 'blk3' 0x626c6b33 (:6)
 *   BeginContext / Hash / EndContext<-> Blake3Hash_BeginContext/_Hash/_EndContext (:24-79)
 *   HashBuffer                      <-> Blake3Hash_HashBuffer        (:81-102)
 *
 * HashBuffer first asks the chunk-window registry: when (data,len) is a range handed out by a HIP chunker the
 * digest was already computed on the GPU together with the cut points and is returned without touching the
 * bytes again.  Anything else (path strings src/longtail.c:1272, per-asset chunk-hash arrays :2522, block hash
 * arrays :3757, ranges from a CPU chunker) is copied to the device and hashed there; there is no CPU
 * implementation of BLAKE3 in this library.
 *
 * The object is written once over a table of device calls (struct ltp_hash_kind): BLAKE3's is below, BLAKE2s's -- the 'blk2'
 * object, Longtail_CreateHipBlake2HashAPI -- in plugin_blake2.c.
 */
#include "plugin_common.h"

#define LONGTAIL_HIP_BLAKE3_ID ((((uint32_t)'b') << 24) + (((uint32_t)'l') << 16) + (((uint32_t)'k') << 8) + ((uint32_t)'3'))

struct HipHashAPI
{
    struct Longtail_HashAPI api;
    const struct ltp_hash_kind* kind;
};

/* Streaming context: O(1) host memory whatever the stream's length (the reference's blake3_hasher is 1 912 bytes; round 2 buffered the
 * WHOLE stream on the host and stopped at 4 GiB).  One batch of LTHIP_B3_STREAM_BATCH bytes is collected on the host; when it is full
 * AND another byte arrives it goes to the device, is reduced to its subtree's chaining value and merged into the stream's stack,
 * which lives in device memory (lthip_b3_stream_batch).  EndContext sends what is left and folds the stack (lthip_b3_stream_final). */
struct HipHashContext
{
    uint8_t* buf;      /* LTHIP_B3_STREAM_BATCH bytes, allocated with the first Hash() call */
    uint32_t have;     /* bytes in buf */
    uint64_t batches;  /* batches already on the device */
    void* d_stack;     /* device: the stream's subtree stack (BLAKE3) or chaining state (BLAKE2s), allocated with the first batch */
    void* d_batch;     /* device: one batch */
    int err; /* first failure of a Hash() call on this context: EndContext reports it through the error latch */
    const struct ltp_hash_kind* kind;
};

#define LTP_HASH_ONE_MAX 65536u

static int gpu_hash(const struct ltp_hash_kind* kind, const void* data, uint32_t length, uint64_t* out_hash)
{
    struct ltp_thread_state* ts = ltp_thread_state_get();
    if (!ts)
        return ENODEV;
    lthip_ctx* ctx = ts->ctx;
    if (length <= LTP_HASH_ONE_MAX)
    {
        /* small inputs (paths, hash arrays): copied into the thread's pinned block, hashed from there by ONE launch that also
         * writes the digest back into it -- no upload, no download, one synchronisation */
        const size_t data_bytes = ((size_t)length + 15u) & ~(size_t)15u;
        int err = ltp_pin_reserve(ctx, &ts->h_pin, data_bytes + 64);
        if (err)
            return err;
        uint8_t* h = (uint8_t*)ts->h_pin.p;
        if (length)
            memcpy(h, data, length);
        uint64_t* res = (uint64_t*)(h + data_bytes);
        err = kind->one(ctx, h, length, res);
        if (!err)
            err = lthip_ctx_sync(ctx);
        if (err)
            return err;
        *out_hash = *res;
        return 0;
    }
    /* layout of d_in: [data, padded to 16][u64 offset][u32 len][pad][u64 hash] */
    const size_t data_bytes = ((size_t)length + 15u) & ~(size_t)15u;
    int err = ltp_dev_reserve(ctx, &ts->d_in, data_bytes + 64);
    if (!err)
        err = ltp_pin_reserve(ctx, &ts->h_pin, 64);
    if (err)
        return err;
    uint8_t* d = (uint8_t*)ts->d_in.p;
    uint64_t* h_tab = (uint64_t*)ts->h_pin.p;
    h_tab[0] = 0;                  /* offset */
    ((uint32_t*)h_tab)[2] = length; /* len at byte 8 */
    err = lthip_copy_h2d(ctx, d, data, length);
    if (!err)
        err = lthip_copy_h2d(ctx, d + data_bytes, h_tab, 16);
    if (!err)
        err = kind->ranges(ctx, d, 1, (const uint64_t*)(d + data_bytes), (const uint32_t*)(d + data_bytes + 8), length,
                           (uint64_t*)(d + data_bytes + 16));
    if (!err)
        err = lthip_copy_d2h(ctx, &h_tab[4], d + data_bytes + 16, 8);
    if (!err)
        err = lthip_ctx_sync(ctx);
    if (err)
        return err;
    *out_hash = h_tab[4];
    return 0;
}

static int b3_stream_final(lthip_ctx* ctx, const void* d_tail, uint32_t tail_len, uint64_t batch_count, void* d_stack, uint64_t* d_out)
{
    return lthip_b3_stream_final(ctx, d_tail, tail_len, batch_count, d_stack, d_out);
}

static const struct ltp_hash_kind g_blake3 = {LONGTAIL_HIP_BLAKE3_ID, lthip_hash_one, lthip_hash_ranges, lthip_b3_stream_batch,
                                              b3_stream_final, LTHIP_B3_STREAM_STACK_BYTES, 1, 0};

static uint32_t HipHash_GetIdentifier(struct Longtail_HashAPI* hash_api)
{
    return hash_api ? ((struct HipHashAPI*)hash_api)->kind->id : 0;
}

static int HipHash_BeginContext(struct Longtail_HashAPI* hash_api, Longtail_HashAPI_HContext* out_context)
{
    if (!hash_api || !out_context)
        return EINVAL;
    struct HipHashContext* c = (struct HipHashContext*)ltp_alloc("HipHash_BeginContext", sizeof *c);
    if (!c)
        return ENOMEM;
    memset(c, 0, sizeof *c);
    c->kind = ((struct HipHashAPI*)hash_api)->kind;
    *out_context = (Longtail_HashAPI_HContext)c;
    return 0;
}

static int stream_flush_batch(struct HipHashContext* c, lthip_ctx* ctx)
{
    int err = 0;
    if (!c->d_batch)
        err = lthip_malloc_device(ctx, LTHIP_B3_STREAM_BATCH, &c->d_batch);
    if (!err && !c->d_stack)
        err = lthip_malloc_device(ctx, c->kind->stream_state_bytes, &c->d_stack);
    if (!err)
        err = lthip_copy_h2d(ctx, c->d_batch, c->buf, LTHIP_B3_STREAM_BATCH);
    if (!err)
        err = c->kind->stream_batch(ctx, c->d_batch, c->batches, c->d_stack);
    if (!err)
        err = lthip_ctx_sync(ctx); /* the host buffer is refilled next, and the next call may come from another thread */
    if (!err)
    {
        c->batches += 1;
        c->have = 0;
    }
    return err;
}

static void HipHash_Hash(struct Longtail_HashAPI* hash_api, Longtail_HashAPI_HContext context, uint32_t length,
                         const void* data)
{
    struct HipHashContext* c = (struct HipHashContext*)context;
    if (!hash_api || !c || !length || !data || c->err)
        return;
    /* a void function in the ABI (src/longtail.h:205): a failure is remembered and surfaces at EndContext, which then returns 0
     * and latches the errno (Longtail_Hip_GetLastError) instead of the digest of a truncated stream */
    if (!c->buf)
    {
        c->buf = (uint8_t*)ltp_alloc("HipHash_Hash", LTHIP_B3_STREAM_BATCH);
        if (!c->buf)
        {
            c->err = ENOMEM;
            ltp_latch_error(ENOMEM);
            return;
        }
    }
    const uint8_t* p = (const uint8_t*)data;
    while (length)
    {
        if (c->have == LTHIP_B3_STREAM_BATCH)
        {
            /* the batch is full and more follows: it is not the end of the stream */
            lthip_ctx* ctx = ltp_thread_ctx();
            const int err = ctx ? stream_flush_batch(c, ctx) : ENODEV;
            if (err)
            {
                c->err = err;
                ltp_latch_error(err);
                return;
            }
        }
        uint32_t n = LTHIP_B3_STREAM_BATCH - c->have;
        if (n > length)
            n = length;
        memcpy(c->buf + c->have, p, n);
        c->have += n;
        p += n;
        length -= n;
    }
}

static uint64_t HipHash_EndContext(struct Longtail_HashAPI* hash_api, Longtail_HashAPI_HContext context)
{
    struct HipHashContext* c = (struct HipHashContext*)context;
    uint64_t h = 0;
    if (!hash_api || !c)
        return 0;
    int err = c->err;
    lthip_ctx* ctx = 0;
    if (!err)
    {
        struct ltp_thread_state* ts = ltp_thread_state_get();
        ctx = ts ? ts->ctx : 0;
        if (!ctx)
            err = ENODEV;
        else if (c->batches == 0 && c->have <= LTP_HASH_ONE_MAX)
            err = gpu_hash(c->kind, c->buf ? c->buf : (const uint8_t*)"", c->have, &h); /* a short stream is a HashBuffer */
        else
        {
            /* the rest of the stream (1 .. one batch of bytes) and the fold of the stack, digest into the thread's pinned block */
            if (!c->d_batch)
                err = lthip_malloc_device(ctx, LTHIP_B3_STREAM_BATCH, &c->d_batch);
            if (!err)
                err = ltp_pin_reserve(ctx, &ts->h_pin, 64);
            if (!err)
                err = lthip_copy_h2d(ctx, c->d_batch, c->buf, c->have);
            if (!err)
                err = c->kind->stream_final(ctx, c->d_batch, c->have, c->batches, c->d_stack, (uint64_t*)ts->h_pin.p);
            if (!err)
                err = lthip_ctx_sync(ctx);
            if (!err)
                h = *(const uint64_t*)ts->h_pin.p;
        }
    }
    if (err)
    {
        /* never a plausible digest for a stream that could not be hashed: 0 + the errno in the latch */
        ltp_latch_error(err);
        h = 0;
    }
    if (!ctx)
        ctx = ltp_thread_ctx();
    if (ctx)
    {
        lthip_free_device(ctx, c->d_batch);
        lthip_free_device(ctx, c->d_stack);
    }
    ltp_free(c->buf);
    ltp_free(c);
    return h;
}

static int HipHash_HashBuffer(struct Longtail_HashAPI* hash_api, uint32_t length, const void* data, uint64_t* out_hash)
{
    if (!hash_api || !data || !out_hash)
        return EINVAL; /* longtail_blake3.c:94-96 */
    const struct ltp_hash_kind* kind = ((struct HipHashAPI*)hash_api)->kind;
    if (!kind->use_windows)
    {
        /* the window registry and the memo hold BLAKE3 digests: the kind's own table of the chunker's window, else the GPU */
        const int hit = kind->window_lookup && length ? kind->window_lookup(kind, data, length, out_hash) : 0;
        if (hit < 0)
            return -hit;
        return hit ? 0 : gpu_hash(kind, data, length, out_hash);
    }
    if (length && ltp_window_lookup(data, length, out_hash))
        return 0;
    if (ltp_memo_get(data, length, out_hash)) /* an asset's digest array the batcher has hashed on the GPU already */
        return 0;
    return gpu_hash(kind, data, length, out_hash);
}

struct window_table_arg
{
    const struct ltp_hash_kind* kind;
    uint64_t* out_hash;
};

static int window_table_digest(const struct ltp_window* pub, uint32_t index, void* varg)
{
    const struct window_table_arg* arg = (const struct window_table_arg*)varg;
    struct ltp_chunk_window* w = pub->owner;
    if (w->hash2_id != arg->kind->id)
    {
        lthip_ctx* ctx = ltp_thread_ctx();
        if (!ctx)
            return -ENODEV;
        int err = 0;
        w->hash2_id = 0; /* a failure below leaves no kind's table */
        if (!w->h_hash2)
            err = lthip_malloc_pinned(ctx, (size_t)w->ccap * 8, (void**)&w->h_hash2);
        if (!err && !w->d_resident)
        {
            err = lthip_copy_h2d(ctx, w->d_win, pub->base, (size_t)pub->size);
            if (!err) err = lthip_copy_h2d(ctx, w->d_off, pub->offsets, (size_t)pub->count * 8);
            if (!err) err = lthip_copy_h2d(ctx, w->d_len, pub->lens, (size_t)pub->count * 4);
        }
        if (!err) err = arg->kind->ranges(ctx, w->d_win, pub->count, w->d_off, w->d_len, w->max_chunk, w->d_hash);
        if (!err) err = lthip_copy_d2h(ctx, w->h_hash2, w->d_hash, (size_t)pub->count * 8);
        if (!err) err = lthip_ctx_sync(ctx);
        if (err)
            return -err;
        w->hash2_id = arg->kind->id;
    }
    *arg->out_hash = w->h_hash2[index];
    return 1;
}

int ltp_window_table_lookup(const struct ltp_hash_kind* kind, const void* data, uint32_t len, uint64_t* out_hash)
{
    struct window_table_arg arg = {kind, out_hash};
    const int r = ltp_window_with_current(data, len, window_table_digest, &arg);
    return r < 0 && r != -1 ? r : (r == 1);
}

static void HipHash_Dispose(struct Longtail_API* api) { ltp_free(api); }

struct Longtail_HashAPI* ltp_create_hash_api(const struct ltp_hash_kind* kind)
{
    if (lthip_device_count() <= 0)
        return 0; /* no GPU: fail loudly */
    struct HipHashAPI* a = (struct HipHashAPI*)ltp_alloc("HipHashAPI", sizeof *a);
    if (!a)
        return 0;
    a->kind = kind;
    a->api.m_API.Dispose = HipHash_Dispose;
    a->api.GetIdentifier = HipHash_GetIdentifier;
    a->api.BeginContext = HipHash_BeginContext;
    a->api.Hash = HipHash_Hash;
    a->api.EndContext = HipHash_EndContext;
    a->api.HashBuffer = HipHash_HashBuffer;
    return &a->api;
}

struct Longtail_HashAPI* Longtail_CreateHipBlake3HashAPI(void) { return ltp_create_hash_api(&g_blake3); }
