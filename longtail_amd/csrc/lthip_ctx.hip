// lthip_ctx.hip -- context, scratch pools, per-kernel event timing, plans and the phase-1 orchestration
// of liblongtail_hip.so.  Host code only; the kernels live in k_*.hip.
#include "lthip_internal.h"
#include "store_index_ops.h"

#include <stdlib.h>

#include <new>

// ---------------------------------------------------------------------------------------------------
// errors / scratch
// ---------------------------------------------------------------------------------------------------
int lthip_fail(lthip_ctx* ctx, int code, const char* what, const char* detail)
{
    if (ctx)
        snprintf(ctx->err, sizeof ctx->err, "%s: %s", what ? what : "?", detail ? detail : "");
    return code;
}

int lthip_scratch(lthip_ctx* ctx, int slot, size_t bytes, void** out)
{
    if (bytes == 0)
        bytes = 256;
    if (ctx->scratch_cap[slot] < bytes)
    {
        if (ctx->scratch[slot])
        {
            // the old buffer may still be in use by work queued on the stream
            LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
            LTHIP_CHECK(ctx, hipFree(ctx->scratch[slot]));
            ctx->scratch[slot] = nullptr;
            ctx->scratch_cap[slot] = 0;
        }
        size_t cap = bytes + bytes / 8 + 4096; // head-room so slowly growing batches do not realloc
        LTHIP_CHECK(ctx, lthip_hip_malloc(&ctx->scratch[slot], cap));
        ctx->scratch_cap[slot] = cap;
    }
    *out = ctx->scratch[slot];
    return 0;
}

volatile uint32_t g_lthip_env_gen = 1;
extern "C" void lthip_debug_reload_env(void) { g_lthip_env_gen = g_lthip_env_gen + 1u; }

// ---- allocation-failure injection (ablation build only; the product build answers ENOTSUP and has no counter in its allocation path) ----
#ifdef LTHIP_ABLATIONS
namespace
{
std::atomic<int64_t> g_alloc_calls{0};            // allocations attempted by this process (both kinds)
std::atomic<int64_t> g_fail_first{INT64_MAX};     // 1-based number of the first allocation that fails
std::atomic<int64_t> g_fail_last{INT64_MAX};      // ... and of the last one (inclusive)
std::atomic<int64_t> g_alloc_failed{0};           // how many were made to fail
bool inject_failure()
{
    const int64_t n = g_alloc_calls.fetch_add(1, std::memory_order_relaxed) + 1;
    if (n < g_fail_first.load(std::memory_order_relaxed) || n > g_fail_last.load(std::memory_order_relaxed))
        return false;
    g_alloc_failed.fetch_add(1, std::memory_order_relaxed);
    return true;
}
} // namespace
hipError_t lthip_hip_malloc(void** p, size_t bytes)
{
    if (inject_failure())
    {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    return hipMalloc(p, bytes);
}
hipError_t lthip_hip_host_malloc(void** p, size_t bytes, unsigned flags)
{
    if (inject_failure())
    {
        *p = nullptr;
        return hipErrorOutOfMemory;
    }
    return hipHostMalloc(p, bytes, flags);
}
extern "C" int lthip_debug_fail_alloc(int64_t after, int64_t count)
{
    if (after < 0 || count <= 0)
    {
        g_fail_first = INT64_MAX; // off
        g_fail_last = INT64_MAX;
        return 0;
    }
    const int64_t now = g_alloc_calls.load();
    g_fail_last = INT64_MAX;
    g_fail_first = now + after + 1;
    g_fail_last = count > INT64_MAX - (now + after) ? INT64_MAX : now + after + count;
    return 0;
}
extern "C" int64_t lthip_debug_alloc_calls(int64_t* out_failed)
{
    if (out_failed)
        *out_failed = g_alloc_failed.load();
    return g_alloc_calls.load();
}
#else
extern "C" int lthip_debug_fail_alloc(int64_t, int64_t) { return ENOTSUP; }
extern "C" int64_t lthip_debug_alloc_calls(int64_t* out_failed)
{
    if (out_failed)
        *out_failed = 0;
    return -1;
}
#endif

// ---------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------
extern "C" int lthip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

extern "C" int lthip_ctx_create(int device, void* hip_stream, lthip_ctx** out_ctx)
{
    if (!out_ctx)
        return EINVAL;
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return ENODEV; // fail loudly: there is no CPU fallback in this library
    if (device < 0 || device >= n)
        return EINVAL;
    if (hipSetDevice(device) != hipSuccess)
        return EIO;
    lthip_ctx* ctx = new (std::nothrow) lthip_ctx();
    if (!ctx)
        return ENOMEM;
    ctx->device = device;
    ctx->slice_ctx = nullptr;
    ctx->err[0] = 0;
    ctx->timing = false;
    memset(ctx->scratch, 0, sizeof ctx->scratch);
    memset(ctx->stage, 0, sizeof ctx->stage);
    memset(ctx->stage_small, 0, sizeof ctx->stage_small);
    ctx->stage_next = ctx->stage_small_next = 0;
    ctx->z_last_retry = nullptr;
    ctx->z_last_payloads = 0;
    ctx->z_last_foreign_blocks = 0;
    memset(ctx->k5_lds_enabled, 0, sizeof ctx->k5_lds_enabled);
    memset(ctx->scratch_cap, 0, sizeof ctx->scratch_cap);
    memset(ctx->total_ms, 0, sizeof ctx->total_ms);
    memset(ctx->launches, 0, sizeof ctx->launches);
    if (hip_stream != LTHIP_STREAM_PRIVATE)
    {
        ctx->stream = (hipStream_t)hip_stream; // may be the null stream
        ctx->own_stream = false;
    }
    else
    {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess)
        {
            delete ctx;
            return EIO;
        }
        ctx->own_stream = true;
    }
    *out_ctx = ctx;
    return 0;
}

hipError_t lthip_stream_wait(lthip_ctx* ctx) { return hipStreamSynchronize(ctx->stream); }

// How host threads wait for this device: hipDeviceScheduleBlockingSync (a waiting thread sleeps until the interrupt) instead of the
// runtime's default, which polls the completion signal.  The plugin layer's callers are the embedder's job-system workers, 32-256
// threads each blocked in a Longtail_*API call: polling was a third of the drop-in path's CPU time, and in a container with a CPU
// quota (the measured boxes grant 16 CPUs of 256: cgroup cpu.max) CPU time IS that path's throughput -- CreateVersionIndex through the
// plugins 30 -> 40 GB/s at 32 workers, 16-20 -> 39 at 64 (tools/dropin_scaling.py, profiles/r06_dropin_scaling.txt).
// It is the DEVICE's policy, process-wide, and it has to be set BEFORE the process uses the device: switched in a process that had
// already run kernels and sessions, a later event wait of the ingest session never returned (bench.py, round 6: the completion signals
// made under the polling policy do not interrupt).  So the library never sets it on its own: Longtail_Hip_SetBlockingWaits(1) is the
// embedder's FIRST call (include/longtail_hip.h).  Measured and not used instead: an event made with hipEventBlockingSync in place of
// hipStreamSynchronize (polls like the default), hipStreamQuery + nanosleep (user time 8.5 -> 2.5 s but the timer slack's 50 us per wait
// cost more than the CPU time bought: 12.4 GB/s of UpSync against 13.9 with the default and 15.5-16.5 with the policy).
extern "C" int lthip_set_blocking_waits(int device, int on)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return ENODEV;
    int prev = 0;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess)
        return EIO;
    const hipError_t e = hipSetDeviceFlags(on ? hipDeviceScheduleBlockingSync : hipDeviceScheduleAuto);
    (void)hipSetDevice(prev);
    return e == hipSuccess ? 0 : EIO;
}

extern "C" void lthip_ctx_destroy(lthip_ctx* ctx)
{
    if (!ctx)
        return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->slice_ctx)
        lthip_ctx_destroy(ctx->slice_ctx);
    for (auto& r : ctx->pending)
    {
        (void)hipEventDestroy(r.a);
        (void)hipEventDestroy(r.b);
    }
    for (auto e : ctx->free_events)
        (void)hipEventDestroy(e);
    for (auto e : ctx->sync_events)
        (void)hipEventDestroy(e);
    if (ctx->stream2)
    {
        (void)hipStreamSynchronize(ctx->stream2);
        (void)hipStreamDestroy(ctx->stream2);
    }
    for (int i = 0; i < S_COUNT; ++i)
        if (ctx->scratch[i])
            (void)hipFree(ctx->scratch[i]);
    for (auto& st : ctx->stage)
    {
        if (st.done)
            (void)hipEventDestroy(st.done);
        if (st.p)
            (void)hipHostFree(st.p);
    }
    for (auto& st : ctx->stage_small)
    {
        if (st.done)
            (void)hipEventDestroy(st.done);
        if (st.p)
            (void)hipHostFree(st.p);
    }
    if (ctx->own_stream)
        (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" int lthip_ctx_sync(lthip_ctx* ctx)
{
    if (!ctx)
        return EINVAL;
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    return 0;
}

extern "C" const char* lthip_ctx_error(const lthip_ctx* ctx) { return ctx ? ctx->err : "no context"; }

// ---------------------------------------------------------------------------------------------------
// memory helpers for plain-C callers
// ---------------------------------------------------------------------------------------------------
extern "C" int lthip_malloc_device(lthip_ctx* ctx, size_t bytes, void** out)
{
    if (!ctx || !out)
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LTHIP_CHECK(ctx, lthip_hip_malloc(out, bytes ? bytes : 16));
    return 0;
}

extern "C" void lthip_free_device(lthip_ctx* ctx, void* p)
{
    if (!p)
        return;
    if (ctx)
    {
        (void)hipSetDevice(ctx->device);
        (void)lthip_stream_wait(ctx);
    }
    (void)hipFree(p);
}

extern "C" int lthip_malloc_pinned(lthip_ctx* ctx, size_t bytes, void** out)
{
    if (!ctx || !out)
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LTHIP_CHECK(ctx, lthip_hip_host_malloc(out, bytes ? bytes : 16, hipHostMallocDefault));
    return 0;
}

extern "C" void lthip_free_pinned(lthip_ctx* ctx, void* p)
{
    if (!p)
        return;
    if (ctx)
    {
        (void)hipSetDevice(ctx->device);
        (void)lthip_stream_wait(ctx);
    }
    (void)hipHostFree(p);
}

extern "C" int lthip_copy_h2d(lthip_ctx* ctx, void* d_dst, const void* h_src, size_t bytes)
{
    if (!ctx || (bytes && (!d_dst || !h_src)))
        return EINVAL;
    if (bytes == 0)
        return 0;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LTHIP_CHECK(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

extern "C" int lthip_copy_d2h(lthip_ctx* ctx, void* h_dst, const void* d_src, size_t bytes)
{
    if (!ctx || (bytes && (!h_dst || !d_src)))
        return EINVAL;
    if (bytes == 0)
        return 0;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    LTHIP_CHECK(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------------------------------
static hipEvent_t take_event(lthip_ctx* ctx)
{
    if (!ctx->free_events.empty())
    {
        hipEvent_t e = ctx->free_events.back();
        ctx->free_events.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

LaunchTimer::LaunchTimer(lthip_ctx* c, int kid, hipStream_t s) : ctx(c), on(c->timing), stream(s ? s : c->stream)
{
    if (on)
    {
        rec.kid = kid;
        rec.a = take_event(ctx);
        rec.b = take_event(ctx);
        (void)hipEventRecord(rec.a, stream);
    }
}

int lthip_second_stream(lthip_ctx* ctx, hipStream_t* out)
{
    if (!ctx->stream2)
        LTHIP_CHECK(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    *out = ctx->stream2;
    return 0;
}

int lthip_stage_upload(lthip_ctx* ctx, void* d_dst, const void* h_src, size_t bytes, hipStream_t stream)
{
    if (bytes == 0)
        return 0;
    const bool small = bytes <= LTHIP_STAGE_SMALL;
    LTHIP_ABLATION_ENV(env_slots, "LTHIP_STAGE_SLOTS"); // (experiment: 8 = the ring of rounds 1-2)
    const size_t nsmall = env_slots.get() > 0 && env_slots.get() < 64 ? (size_t)env_slots.get() : sizeof(ctx->stage_small) / sizeof(ctx->stage_small[0]);
    lthip_ctx::Stage& st = small ? ctx->stage_small[ctx->stage_small_next++ % nsmall]
                                 : ctx->stage[ctx->stage_next++ % (sizeof(ctx->stage) / sizeof(ctx->stage[0]))];
    if (st.used)
        LTHIP_CHECK(ctx, hipEventSynchronize(st.done)); // a ring ago: long finished in steady state
    if (st.cap < bytes)
    {
        if (st.p)
            LTHIP_CHECK(ctx, hipHostFree(st.p));
        st.p = nullptr;
        st.cap = 0;
        const size_t want = small ? LTHIP_STAGE_SMALL : bytes + bytes / 2 + 4096;
        LTHIP_CHECK(ctx, lthip_hip_host_malloc(&st.p, want, hipHostMallocDefault));
        st.cap = want;
    }
    if (!st.done)
        LTHIP_CHECK(ctx, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    memcpy(st.p, h_src, bytes);
    LTHIP_CHECK(ctx, hipMemcpyAsync(d_dst, st.p, bytes, hipMemcpyHostToDevice, stream));
    LTHIP_CHECK(ctx, hipEventRecord(st.done, stream));
    st.used = true;
    return 0;
}

hipEvent_t lthip_sync_event(lthip_ctx* ctx)
{
    // 16 events in rotation: an event is re-recorded only long after the wait that used it has been queued behind
    // newer work on both streams
    if (ctx->sync_events.size() < 16)
    {
        hipEvent_t e = nullptr;
        (void)hipEventCreateWithFlags(&e, hipEventDisableTiming);
        ctx->sync_events.push_back(e);
        return e;
    }
    return ctx->sync_events[ctx->sync_next++ % ctx->sync_events.size()];
}

LaunchTimer::~LaunchTimer()
{
    if (on)
    {
        (void)hipEventRecord(rec.b, stream);
        ctx->pending.push_back(rec);
    }
}

static int timing_collect(lthip_ctx* ctx)
{
    if (ctx->pending.empty())
        return 0;
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    for (auto& r : ctx->pending)
    {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess)
        {
            ctx->total_ms[r.kid] += (double)ms;
            ctx->launches[r.kid] += 1;
        }
        ctx->free_events.push_back(r.a);
        ctx->free_events.push_back(r.b);
    }
    ctx->pending.clear();
    return 0;
}

extern "C" int lthip_timing_enable(lthip_ctx* ctx, int on)
{
    if (!ctx)
        return EINVAL;
    int err = timing_collect(ctx);
    ctx->timing = on != 0;
    if (ctx->slice_ctx)
        (void)lthip_timing_enable(ctx->slice_ctx, on);
    return err;
}

extern "C" int lthip_timing_reset(lthip_ctx* ctx)
{
    if (!ctx)
        return EINVAL;
    int err = timing_collect(ctx);
    memset(ctx->total_ms, 0, sizeof ctx->total_ms);
    memset(ctx->launches, 0, sizeof ctx->launches);
    if (ctx->slice_ctx)
        (void)lthip_timing_reset(ctx->slice_ctx);
    return err;
}

extern "C" int lthip_timing_get(lthip_ctx* ctx, int kernel_id, double* out_total_ms, uint64_t* out_launches)
{
    if (!ctx || kernel_id < 0 || kernel_id >= LTHIP_K_COUNT)
        return EINVAL;
    int err = timing_collect(ctx);
    double ms = ctx->total_ms[kernel_id];
    uint64_t n = ctx->launches[kernel_id];
    if (ctx->slice_ctx) // (slices 1 .. S-1 of lthip_chunk_hash run on a context of their own: their launches count here)
    {
        double ms2 = 0;
        uint64_t n2 = 0;
        if (lthip_timing_get(ctx->slice_ctx, kernel_id, &ms2, &n2) == 0)
        {
            ms += ms2;
            n += n2;
        }
    }
    if (out_total_ms)
        *out_total_ms = ms;
    if (out_launches)
        *out_launches = n;
    return err;
}

// ---------------------------------------------------------------------------------------------------
// plans
// ---------------------------------------------------------------------------------------------------
// hpcdcchunker.c:126-129 -- the one floating-point step of the path, evaluated on the host in double
// exactly like the reference.
static uint32_t discriminator_from_avg(uint32_t avg)
{
    double a = (double)avg;
    return (uint32_t)(a / (-1.42888852e-7 * a + 1.33237515));
}

// Division-free form of the reference's cut test `hash % d == d-1` (hpcdcchunker.c:298).
//   h % d == d-1  <=>  x = h+1 (as an integer in [1, 2^32]) is a multiple of d.
// Write d = dodd * 2^k2, inv = dodd^-1 (mod 2^32).  Multiplication by inv permutes Z/2^32 and maps the
// multiples of dodd onto [0, floor((2^32-1)/dodd)], so for x in [1, 2^32-1]:
//   d | x  <=>  M = x*inv (mod 2^32) has k2 trailing zero bits and 1 <= M >> k2 <= q,  q = floor((2^32-1)/d)
//          <=>  ror32(M - 2^k2, k2) <= q-1          (a wrong low bit, or M = 0, lands in the top bits)
// and M - 2^k2 = h*inv + (inv - 2^k2), one multiply-add.  x = 2^32 (h = 0xFFFFFFFF) gives M = 0, which is
// rejected -- correct unless d is a power of two, which gets its own mask test.
static DivTest make_div_test(uint32_t d)
{
    DivTest t;
    memset(&t, 0, sizeof t);
    t.d = d;
    if (d == 0)
        return t; // rejected by plan_create
    uint32_t k2 = 0, dodd = d;
    while ((dodd & 1u) == 0)
    {
        dodd >>= 1;
        ++k2;
    }
    uint32_t inv = dodd; // Newton iteration, 5 steps give 32 bits
    for (int i = 0; i < 5; ++i)
        inv *= 2u - dodd * inv;
    t.inv = inv;
    t.k2 = k2;
    t.addc = inv - (1u << k2);
    t.qlim = (uint32_t)(0xFFFFFFFFull / d) - 1u;
    t.pow2 = dodd == 1u;
    return t;
}

// Greedy block packing of Longtail_CreateStoreIndex (src/longtail.c:6801-6860): host control logic, serial in the
// reference as well.  block_starts receives block_count+1 chunk indices.
extern "C" int lthip_pack_blocks(uint64_t chunk_count, const uint32_t* chunk_lens, uint32_t max_block_size,
                                 uint32_t max_chunks_per_block, uint64_t* block_starts, uint64_t capacity, uint64_t* out_block_count)
{
    if (!out_block_count || (chunk_count && (!chunk_lens || !block_starts)) || max_block_size == 0 || max_chunks_per_block == 0)
        return EINVAL;
    const uint64_t limit = (uint64_t)max_block_size + max_block_size / 10; // "overshoot by 10% is ok"
    uint64_t i = 0, nb = 0;
    while (i < chunk_count)
    {
        if (nb + 1 >= capacity)
            return ENOMEM;
        block_starts[nb++] = i;
        uint64_t size = chunk_lens[i];
        uint32_t n = 1;
        while (i + 1 < chunk_count && n < max_chunks_per_block && size + chunk_lens[i + 1] <= limit)
        {
            size += chunk_lens[i + 1];
            ++n;
            ++i;
        }
        ++i;
    }
    if (capacity == 0)
        return ENOMEM;
    block_starts[nb] = chunk_count;
    *out_block_count = nb;
    return 0;
}

// The same rule, resumable: packs blocks from chunk `first_chunk` on until the batch holds max_batch_bytes of chunk data
// or its codec output bounds (size + size / bound_div + bound_add, rounded up to 64) fill arena_bytes -- always at least
// one block -- so that a caller can hand batch k to the device and pack batch k+1 while it is being compressed.
extern "C" int lthip_pack_blocks_batch(uint64_t chunk_count, const uint32_t* chunk_lens, uint64_t first_chunk,
                                       uint32_t max_block_size, uint32_t max_chunks_per_block, uint64_t max_batch_bytes,
                                       uint64_t arena_bytes, uint32_t bound_div, uint32_t bound_add, uint64_t* block_starts,
                                       uint64_t* block_sizes, uint64_t capacity, uint64_t* out_block_count,
                                       uint64_t* out_next_chunk)
{
    if (!out_block_count || !out_next_chunk || !block_starts || !block_sizes || (chunk_count && !chunk_lens) ||
        max_block_size == 0 || max_chunks_per_block == 0 || bound_div == 0 || capacity < 2 || first_chunk > chunk_count)
        return EINVAL;
    const uint64_t limit = (uint64_t)max_block_size + max_block_size / 10;
    uint64_t i = first_chunk, nb = 0, bytes = 0, arena = 0;
    while (i < chunk_count && nb + 1 < capacity)
    {
        const uint64_t start = i;
        uint64_t size = chunk_lens[i];
        uint32_t n = 1;
        while (i + 1 < chunk_count && n < max_chunks_per_block && size + chunk_lens[i + 1] <= limit)
        {
            size += chunk_lens[i + 1];
            ++n;
            ++i;
        }
        ++i;
        const uint64_t bound = (size + size / bound_div + bound_add + 63u) & ~(uint64_t)63u;
        if (nb && (bytes + size > max_batch_bytes || arena + bound > arena_bytes))
        {
            i = start; // this block opens the next batch
            break;
        }
        block_starts[nb] = start;
        block_sizes[nb] = size;
        ++nb;
        bytes += size;
        arena += bound;
    }
    block_starts[nb] = i;
    *out_block_count = nb;
    *out_next_chunk = i;
    return 0;
}

// The index operations of store_index_ops.h behind the C interface: host only, no context.  An allocation that fails is ENOMEM with
// *out_size / *count left as it was.
extern "C" int lthip_store_index_prune(const void* store_index, size_t size, uint32_t keep_count, const uint64_t* keep_block_hashes, void* out,
                                       size_t out_capacity, size_t* out_size)
{
    return lthip_guarded(nullptr, nullptr, [&] { return store_index_ops::prune(store_index, size, keep_count, keep_block_hashes, out, out_capacity, out_size); });
}

extern "C" int lthip_store_index_merge(const void* local, size_t local_size, const void* remote, size_t remote_size, void* out, size_t out_capacity,
                                       size_t* out_size)
{
    return lthip_guarded(nullptr, nullptr, [&] { return store_index_ops::merge(local, local_size, remote, remote_size, out, out_capacity, out_size); });
}

extern "C" int lthip_version_chunk_hashes(const void* version_index, size_t size, uint64_t* out, uint64_t capacity, uint64_t* count)
{
    return store_index_ops::version_chunk_hashes(version_index, size, out, capacity, count);
}

extern "C" int lthip_divtest_eval(uint32_t discriminator, uint32_t hash)
{
    if (discriminator == 0)
        return 0;
    const DivTest t = make_div_test(discriminator);
    if (t.pow2)
        return (hash & (t.d - 1u)) == t.d - 1u;
    const uint32_t m = hash * t.inv + t.addc;
    const uint32_t r = t.k2 ? ((m >> t.k2) | (m << (32u - t.k2))) : m;
    return r <= t.qlim;
}

// where a plan's parts are cut into S runs of about equal bytes: first[0] = 0 < first[1] < ... < first[S] = n; returns S (0 = do not slice)
static uint32_t plan_slice_points(uint32_t part_count, const uint64_t* part_sizes, uint32_t want, uint32_t* first)
{
    if (part_count < 2 || want < 2)
        return 0;
    uint64_t total = 0;
    for (uint32_t p = 0; p < part_count; ++p)
        total += part_sizes[p];
    if (total < LTHIP_SLICE_MIN_BYTES)
        return 0;
    uint32_t S = want > part_count ? part_count : want;
    while (S > 2 && total / S < LTHIP_SLICE_MIN_BYTES / 2)
        --S;
    uint64_t acc = 0;
    uint32_t p = 0;
    first[0] = 0;
    for (uint32_t k = 1; k < S; ++k)
    {
        const uint64_t goal = total / S * k;
        while (p < part_count - (S - k) && acc + part_sizes[p] / 2 < goal)
            acc += part_sizes[p++];
        if (p <= first[k - 1])
        {
            acc += part_sizes[p];
            ++p;
        }
        first[k] = p;
    }
    first[S] = part_count;
    return S;
}

// The one place a plan's layout is computed: checks the parts and fills their device table `parts` and the extents.  `what` is the
// entry point the errors name.
static int plan_layout(lthip_ctx* ctx, const char* what, uint32_t min_chunk, uint32_t part_count, const uint64_t* part_offsets,
                       const uint64_t* part_sizes, PartDev* parts, PlanExtents& x)
{
    memset(&x, 0, sizeof x);
    x.nparts = part_count;
    for (uint32_t p = 0; p < part_count; ++p)
    {
        const uint64_t sz = part_sizes[p];
        // (sizes below 4 GiB are load-bearing in K1: the walking scan holds part-relative distances in 32-bit scalars, k_buzhash.hip)
        if ((part_offsets[p] & 15u) != 0 || sz > 0xFFFFFFFFull)
            return lthip_fail(ctx, EINVAL, what, "part offsets must be 16-byte aligned, sizes < 4 GiB");
        PartDev& pd = parts[p];
        memset(&pd, 0, sizeof pd);
        pd.off = part_offsets[p];
        pd.size = sz;
        pd.bm0_base = x.bm0_words;
        pd.bm1_base = x.bm1_words;
        pd.region_base = x.chunk_cap;
        pd.tile_base = (uint32_t)x.ntiles;
        const uint64_t cap = sz ? sz / min_chunk + 1 : 0; // every chunk but the last is >= min bytes
        pd.region_cap = (uint32_t)cap;
        const uint64_t t = div_up_u64(sz, 16384);
        x.ntiles += t;
        x.bm0_words += t * 256; // one 64-bit word per 64-byte run, whole tiles
        x.bm1_words += t * 4;   // one 64-bit word per 4 KiB
        x.chunk_cap += cap;
        x.total_bytes += sz;
        x.leaf_cap += div_up_u64(sz, 1024) + cap;
        x.nonempty_parts += sz != 0;
        x.max_part_bytes = sz > x.max_part_bytes ? sz : x.max_part_bytes;
    }
    return 0;
}

// whether the parts a plan is aimed at suit the walking scan (lthip_internal.h: the rule and its two constants)
static bool plan_walk_rule(const lthip_plan* plan)
{
    const uint64_t waves = lthip_k1_resident_waves(plan->device);
    return plan->nonempty_parts >= LTHIP_WALK_MIN_PARTS_PER_WAVE * waves &&
           plan->max_part_bytes * LTHIP_WALK_MAX_PART_DIV <= plan->total_bytes / waves;
}

static int plan_create_impl(lthip_ctx* ctx, uint32_t part_count, const uint64_t* part_offsets, const uint64_t* part_sizes,
                            uint32_t min_chunk, uint32_t avg_chunk, uint32_t max_chunk, lthip_plan** out_plan)
{
    if (!ctx || !out_plan || (part_count && (!part_offsets || !part_sizes)))
        return EINVAL;
    *out_plan = nullptr;
    // same parameter contract as Longtail_HPCDCCreateChunker (hpcdcchunker.c:143-146)
    if (min_chunk < 48 || min_chunk > avg_chunk || avg_chunk > max_chunk)
        return lthip_fail(ctx, EINVAL, "lthip_plan_create", "need 48 <= min <= avg <= max");
    uint32_t d = discriminator_from_avg(avg_chunk);
    if (d == 0)
        return lthip_fail(ctx, EINVAL, "lthip_plan_create", "discriminator is zero");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    std::vector<PartDev> parts(part_count);
    PlanExtents x;
    int err = plan_layout(ctx, "lthip_plan_create", min_chunk, part_count, part_offsets, part_sizes, parts.data(), x);
    if (err)
        return err;
    if (x.ntiles > 0xFFFFFFF0ull)
        return lthip_fail(ctx, EINVAL, "lthip_plan_create", "batch too large");

    lthip_plan* plan = new (std::nothrow) lthip_plan();
    if (!plan)
        return ENOMEM;
    memset(plan, 0, sizeof *plan);
    static_cast<PlanExtents&>(*plan) = x;
    plan->device = ctx->device;
    plan->min_chunk = min_chunk;
    plan->avg_chunk = avg_chunk;
    plan->max_chunk = max_chunk;
    plan->div = make_div_test(d);
    plan->capacity_bytes = x.total_bytes;
    plan->cap_parts = part_count ? part_count : 1;
    plan->cap_tiles = x.ntiles ? x.ntiles : 1;
    plan->walked = plan_walk_rule(plan);

    hipError_t e = lthip_hip_malloc((void**)&plan->d_parts, sizeof(PartDev) * plan->cap_parts);
    if (e == hipSuccess)
        e = lthip_hip_malloc((void**)&plan->d_tile_part, sizeof(uint32_t) * plan->cap_tiles);
    if (e == hipSuccess && part_count)
        e = hipMemcpyAsync(plan->d_parts, parts.data(), sizeof(PartDev) * part_count, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = lthip_stream_wait(ctx); // `parts` is a local
    if (e != hipSuccess)
    {
        lthip_plan_destroy(ctx, plan);
        return lthip_fail(ctx, e == hipErrorOutOfMemory ? ENOMEM : EIO, "lthip_plan_create", hipGetErrorString(e));
    }
    if ((err = lthip_launch_tile_table(ctx, plan)))
    {
        lthip_plan_destroy(ctx, plan);
        return err;
    }
    *out_plan = plan;
    return 0;
}

// aims a plan at a layout that fits its tables: the part table goes through the pinned staging ring, the tile -> part table is
// rebuilt by its kernel on the stream
static int plan_aim(lthip_ctx* ctx, lthip_plan* plan, const PlanExtents& x, const PartDev* parts)
{
    static_cast<PlanExtents&>(*plan) = x;
    plan->walked = plan_walk_rule(plan);
    const int err = lthip_stage_upload(ctx, plan->d_parts, parts, sizeof(PartDev) * x.nparts, ctx->stream);
    return err ? err : lthip_launch_tile_table(ctx, plan);
}

// The slices of a plan (lthip_chunk_hash): plans of their own over the same bytes, `want` runs of its parts of about equal bytes.
// The first aim that slices creates them; a later aim re-aims them when the new parts fit them (they do when the layout is the one
// the plan was created with: bench.py's steps), otherwise that aim runs as one.  Optional: a slice that cannot be made or aimed
// leaves the plan unsliced and ctx->err clear, it is never an error of the call.
// A plan whose own scan walks (plan_walks) runs as one unless LTHIP_SLICES of the ablation build names the count: with the walking scan
// a single pass measured faster than any number of slices.  Its slices are still created with it, and kept, but not
// aimed: a later aim at parts that are not walked finds them, as it did when every plan was sliced.
static bool plan_walks(const lthip_plan* plan);
static void plan_aim_slices(lthip_ctx* ctx, lthip_plan* plan, uint32_t want, const uint64_t* part_offsets, const uint64_t* part_sizes)
{
    plan->sliced = false;
    LTHIP_ABLATION_ENV(env_slices, "LTHIP_SLICES");
    const bool as_one = plan_walks(plan) && env_slices.get() <= 0;
    if (as_one && plan->nslices)
        return;
    uint32_t first[9];
    const uint32_t S = plan_slice_points(plan->nparts, part_sizes, want, first);
    if (S == 0 || (plan->nslices && S != plan->nslices))
        return;
    bool ok = true;
    if (!plan->nslices)
        for (uint32_t k = 0; k < S && ok; ++k)
            ok = plan_create_impl(ctx, first[k + 1] - first[k], part_offsets + first[k], part_sizes + first[k], plan->min_chunk,
                                  plan->avg_chunk, plan->max_chunk, &plan->slice[k]) == 0;
    else
    {
        std::vector<PartDev> parts(plan->nparts); // slice k's table at first[k]
        PlanExtents x[8];
        for (uint32_t k = 0; k < S && ok; ++k)
        {
            const uint32_t n = first[k + 1] - first[k];
            ok = plan_layout(ctx, "lthip_plan_reaim", plan->min_chunk, n, part_offsets + first[k], part_sizes + first[k], &parts[first[k]],
                             x[k]) == 0 &&
                 n <= plan->slice[k]->cap_parts && x[k].ntiles <= plan->slice[k]->cap_tiles;
        }
        for (uint32_t k = 0; k < S && ok; ++k)
            ok = plan_aim(ctx, plan->slice[k], x[k], &parts[first[k]]) == 0;
    }
    if (!ok)
    {
        if (!plan->nslices) // (slices that were never aimed together: nothing to keep)
            for (uint32_t k = 0; k < S; ++k)
            {
                lthip_plan_destroy(ctx, plan->slice[k]);
                plan->slice[k] = nullptr;
            }
        ctx->err[0] = 0;
        return;
    }
    memcpy(plan->slice_first, first, sizeof(uint32_t) * (S + 1));
    plan->nslices = S;
    plan->sliced = !as_one;
}

extern "C" int lthip_plan_create(lthip_ctx* ctx, uint32_t part_count, const uint64_t* part_offsets,
                                 const uint64_t* part_sizes, uint32_t min_chunk, uint32_t avg_chunk, uint32_t max_chunk,
                                 lthip_plan** out_plan)
{
    int err = plan_create_impl(ctx, part_count, part_offsets, part_sizes, min_chunk, avg_chunk, max_chunk, out_plan);
    if (err)
        return err;
    int want = LTHIP_SLICES;
    LTHIP_ABLATION_ENV(env_slices, "LTHIP_SLICES"); // (ablation build: 1 = the single pass, for profiles of K1 / K3 alone; 2..8)
    if (env_slices.get() > 0)
        want = env_slices.get() > 8 ? 8 : env_slices.get();
    plan_aim_slices(ctx, *out_plan, (uint32_t)want, part_offsets, part_sizes);
    return 0;
}

// A single-part plan sized once for a CAPACITY and re-aimed at the bytes actually present: what the plugin chunker needs (one
// window of varying fill per refill) without two hipMalloc + a kernel + a synchronisation per file.  The tile -> part table of a
// single part is all zeros whatever the size, so only the part descriptor and the host-side extents change.
extern "C" int lthip_plan_resize_single(lthip_ctx* ctx, lthip_plan* plan, uint64_t size)
{
    if (!ctx || !plan || plan->nparts != 1)
        return EINVAL;
    if (size > plan->capacity_bytes)
        return lthip_fail(ctx, EINVAL, "lthip_plan_resize_single", "size above the capacity the plan was created with");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    const uint64_t off = 0;
    PartDev pd;
    PlanExtents x;
    const int err = plan_layout(ctx, "lthip_plan_resize_single", plan->min_chunk, 1, &off, &size, &pd, x);
    if (err)
        return err;
    static_cast<PlanExtents&>(*plan) = x; // (one part: never walked)
    return lthip_stage_upload(ctx, plan->d_parts, &pd, sizeof pd, ctx->stream);
}

// A plan re-aimed at ANOTHER set of parts (any count up to the one it was created with, any layout whose tiles fit the tile
// table it was created with): no allocation and no synchronisation.  What the plugin layer's batcher needs: one plan, a different
// set of windows in every submission (plugin_batch.c).
extern "C" int lthip_plan_reaim(lthip_ctx* ctx, lthip_plan* plan, uint32_t part_count, const uint64_t* part_offsets,
                                const uint64_t* part_sizes)
{
    if (!ctx || !plan || (part_count && (!part_offsets || !part_sizes)))
        return EINVAL;
    if (part_count == 0 || part_count > plan->cap_parts)
        return lthip_fail(ctx, EINVAL, "lthip_plan_reaim", "part count outside 1 .. the count the plan was created with");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    {
        // (gone before the slices' table is laid out: with both 3 MB tables of the headline plan alive at once, the C library handed
        // their pages back after every aim and the next aim faulted them in again -- 1-2 ms of every step, +30 ms in some)
        std::vector<PartDev> parts(part_count);
        PlanExtents x;
        int err = plan_layout(ctx, "lthip_plan_reaim", plan->min_chunk, part_count, part_offsets, part_sizes, parts.data(), x);
        if (err)
            return err;
        if (x.ntiles > plan->cap_tiles)
            return lthip_fail(ctx, EINVAL, "lthip_plan_reaim", "more 16 KiB tiles than the plan was created with");
        if ((err = plan_aim(ctx, plan, x, parts.data())))
            return err;
    }
    if (plan->nslices)
        plan_aim_slices(ctx, plan, plan->nslices, part_offsets, part_sizes);
    return 0;
}

extern "C" void lthip_plan_destroy(lthip_ctx* ctx, lthip_plan* plan)
{
    if (!plan)
        return;
    // A plan is plain device memory: it may outlive the context (and host thread) that created it.  With a
    // context only its stream is drained; without one the whole device is.
    (void)hipSetDevice(plan->device);
    if (ctx)
        (void)lthip_stream_wait(ctx);
    else
        (void)hipDeviceSynchronize();
    if (plan->d_parts)
        (void)hipFree(plan->d_parts);
    if (plan->d_tile_part)
        (void)hipFree(plan->d_tile_part);
    for (uint32_t k = 0; k < 8; ++k)
        lthip_plan_destroy(ctx, plan->slice[k]);
    delete plan;
}

extern "C" uint64_t lthip_plan_chunk_capacity(const lthip_plan* plan) { return plan ? plan->chunk_cap : 0; }
extern "C" uint32_t lthip_plan_slices(const lthip_plan* plan) { return plan && plan->sliced ? plan->nslices : 1u; }

// whether the scan of (this slice of) a plan is the walking one
static bool plan_walks(const lthip_plan* plan)
{
    LTHIP_ABLATION_ENV(env_walk, "LTHIP_K1_WALK"); // (ablation build: 0 / 1 force the tile scan / the walking scan for any plan)
    if (env_walk.get() >= 0)
        return env_walk.get() != 0 && plan->nparts != 0;
    return plan->walked;
}
extern "C" uint32_t lthip_plan_walked_scans(const lthip_plan* plan)
{
    if (!plan)
        return 0;
    if (!plan->sliced)
        return plan_walks(plan);
    uint32_t n = 0;
    for (uint32_t k = 0; k < plan->nslices; ++k)
        n += plan_walks(plan->slice[k]);
    return n;
}

#ifndef LTHIP_WALK_HASH
#define LTHIP_WALK_HASH 1 // 1: a scan that walks hashes the leaves of the chunks it cuts (k_buzhash_hash_walk); 0: the leaf pass of its own behind it
#endif
// whether the scan of (this slice of) a plan hashes the leaves of its chunks as well: a scan that walks, when hashes are asked for
// (ablation build: LTHIP_WALK_HASH = 0 / 1 forces either form)
static bool plan_walk_hashes(const lthip_plan* plan, bool hashes)
{
    LTHIP_ABLATION_ENV(env_fused, "LTHIP_WALK_HASH");
    const bool on = env_fused.get() >= 0 ? env_fused.get() != 0 : LTHIP_WALK_HASH != 0;
    return on && hashes && plan_walks(plan) && lthip_plan_run_slots(plan) <= 0xFFFFFFF0ull; // (a run's slot is a 32-bit number; the leaf pass has the same limit)
}
uint64_t lthip_plan_run_slots(const lthip_plan* plan) { return plan->chunk_cap + 16u * plan->ntiles; }

// ---------------------------------------------------------------------------------------------------
// phase 1
// ---------------------------------------------------------------------------------------------------
// What the scans of a whole plan leave for cut selection and compaction (the slices' lie back to back in them): the candidate bitmaps
// of the tile scan -- a plan whose scans all walk needs none -- and the bounded chunk region with the per-part counts; with hashes, the
// runs of leaf chaining values of the scans that hash.
struct ScanBuffers
{
    uint64_t *bm0, *bm1;
    uint2* region;
    uint32_t* part_count;
    uint32_t* cv_runs;
};
static int chunk_scan_buffers(lthip_ctx* ctx, const lthip_plan* plan, bool bitmaps, bool hashes, ScanBuffers* b)
{
    b->bm0 = b->bm1 = nullptr;
    b->cv_runs = nullptr;
    int err;
    bool runs = !plan->sliced && plan_walk_hashes(plan, hashes);
    for (uint32_t k = 0; plan->sliced && k < plan->nslices; ++k)
        runs |= plan_walk_hashes(plan->slice[k], hashes);
    if (runs && (err = lthip_scratch(ctx, S_CV_RUNS, lthip_plan_run_slots(plan) * 32, (void**)&b->cv_runs)))
        return err;
    if (bitmaps && ((err = lthip_scratch(ctx, S_BM0, plan->bm0_words * 8, (void**)&b->bm0)) ||
                    (err = lthip_scratch(ctx, S_BM1, plan->bm1_words * 8, (void**)&b->bm1))))
        return err;
    if ((err = lthip_scratch(ctx, S_REGION, plan->chunk_cap * sizeof(uint2), (void**)&b->region)))
        return err;
    return lthip_scratch(ctx, S_PART_COUNT, ((size_t)plan->nparts + 1) * 4, (void**)&b->part_count);
}

// The phase-1 sequence of a plan, in two halves that the sliced pass runs on two streams: the scan -- the tile scan into bm0 / bm1, or
// the walking scan, which selects the cuts as well and leaves the chunk region and the per-part counts ...
static int chunk_scan(lthip_ctx* ctx, const lthip_plan* plan, const void* d_data, const ScanBuffers& b)
{
    if (!plan->nparts)
        return 0;
    return plan_walks(plan) ? lthip_launch_buzhash_walk(ctx, plan, (const uint8_t*)d_data, b.region, b.part_count,
                                                        plan_walk_hashes(plan, b.cv_runs != nullptr) ? b.cv_runs : nullptr)
                            : lthip_launch_buzhash(ctx, plan, (const uint8_t*)d_data, b.bm0, b.bm1);
}

// ... then cut selection (behind a tile scan), compaction and (with d_hashes) the BLAKE3 of the chunks, on ctx's stream behind the scan
static int chunk_cut_hash(lthip_ctx* ctx, const lthip_plan* plan, const void* d_data, const ScanBuffers& b, uint64_t* d_offsets,
                          uint32_t* d_lens, uint64_t* d_hashes, uint32_t* d_part_first)
{
    int err;
    if (plan->nparts && !plan_walks(plan) && (err = lthip_launch_select(ctx, plan, b.bm0, b.bm1, b.region, b.part_count)))
        return err;
    if ((err = lthip_launch_compact(ctx, plan, b.region, b.part_count, d_part_first, d_offsets, d_lens)))
        return err;
    if (!d_hashes)
        return 0;
    if (plan_walk_hashes(plan, b.cv_runs != nullptr)) // the scan has hashed the leaves
        return lthip_launch_blake3_parents(ctx, lthip_b3_runs{b.cv_runs, plan->d_parts, plan->nparts, d_part_first}, d_lens,
                                           d_part_first + plan->nparts, plan->chunk_cap, plan->leaf_cap, plan->max_chunk, d_hashes);
    return lthip_launch_blake3(ctx, (const uint8_t*)d_data, d_offsets, d_lens, d_part_first + plan->nparts, plan->chunk_cap, plan->leaf_cap,
                               plan->max_chunk, d_hashes);
}

// a slice's lists behind the slices before it: base = part_first[0] (= the chunk count of everything before the slice, final by now),
// its lists go to [base, base + total), its part table is shifted by base
__global__ void k_slice_join(const uint64_t* __restrict__ b_off, const uint32_t* __restrict__ b_len, const uint64_t* __restrict__ b_hash,
                             const uint32_t* __restrict__ b_first, uint32_t nparts_b, uint32_t* __restrict__ part_first /* at the slice's first part */,
                             uint64_t* __restrict__ offs, uint32_t* __restrict__ lens, uint64_t* __restrict__ hashes)
{
    const uint32_t base = part_first[0], total_b = b_first[nparts_b];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total_b)
    {
        offs[base + i] = b_off[i];
        lens[base + i] = b_len[i];
        hashes[base + i] = b_hash[i];
    }
    if (i >= 1 && i <= nparts_b) // (entry 0 is the base itself: every thread reads it)
        part_first[i] = b_first[i] + base;
}

// Phase 1 in slices on two streams (plans of >= 1 GiB in >= 2 parts, with hashes).  The candidate scan (K1: four waves per SIMD, its
// issue slots 72 % used, LDS-heavy) and the leaf hashing (K3: VALU bound, no LDS) are both bound by instruction issue and leave each
// other room: with the parts cut into S slices, the scans of the slices run one after the other on the context's stream (scan k + 1
// takes the CUs the moment scan k leaves them: its one workgroup per CU needs 117 KiB of LDS and four waves per SIMD, and would wait
// for a whole grid of hashing workgroups to drain if those got there first) and cut selection, compaction and hashing of every slice
// behind its scan on the slice context's stream -- scan k + 1 beside hashing k.  The lists are the ones of the single pass, bit for
// bit: slice 0 writes the caller's arrays, the others go to scratch and are joined behind it in order (their place depends on the
// counts before them).  tools/k1k3_overlap_probe.py, DESIGN.md §3.
// *taken = false: the plan is not sliced, or what the pass needs could not be had -- nothing was queued, the caller runs the single
// pass.  Once anything is queued every exit joins the second stream into the context's stream, also after a failure.
static int chunk_hash_sliced(lthip_ctx* ctx, const lthip_plan* plan, const void* d_data, uint64_t* d_chunk_offsets, uint32_t* d_chunk_lens, uint64_t* d_chunk_hashes, uint32_t* d_part_first,
                             bool* taken)
{
    *taken = false;
    if (!plan->sliced || !d_chunk_hashes)
        return 0;
    if (!ctx->slice_ctx && lthip_ctx_create(ctx->device, LTHIP_STREAM_PRIVATE, &ctx->slice_ctx) != 0)
        return 0;
    lthip_ctx* c2 = ctx->slice_ctx;
    const uint32_t S = plan->nslices;
    uint64_t cap_rest = 0, parts_rest = 0; // slices 1 .. S-1 in scratch, back to back
    for (uint32_t k = 1; k < S; ++k)
    {
        cap_rest += plan->slice[k]->chunk_cap + 1;
        parts_rest += (uint64_t)plan->slice[k]->nparts + 1;
    }
    void *x_off, *x_len, *x_hash, *x_first;
    ScanBuffers sb; // of the whole plan, on the context: scan k + 1 writes its share while the second stream still reads slice k's
    const bool bitmaps = lthip_plan_walked_scans(plan) != S;
    if (lthip_scratch(ctx, S_SLICE_OFFS, cap_rest * 8, &x_off) || lthip_scratch(ctx, S_SLICE_LENS, cap_rest * 4, &x_len) ||
        lthip_scratch(ctx, S_SLICE_HASH, cap_rest * 8, &x_hash) || lthip_scratch(ctx, S_SLICE_FIRST, parts_rest * 4, &x_first) ||
        chunk_scan_buffers(ctx, plan, bitmaps, true, &sb))
    {
        ctx->err[0] = 0;
        return 0;
    }
    *taken = true;
    c2->timing = ctx->timing;

    int err = 0;
    uint64_t co = 0, po = 0;
    uint64_t *offs_k[8], *hash_k[8];
    uint32_t *lens_k[8], *first_k[8];
    for (uint32_t k = 0; k < S && !err; ++k)
    {
        const lthip_plan* pk = plan->slice[k];
        offs_k[k] = k ? (uint64_t*)x_off + co : d_chunk_offsets;
        lens_k[k] = k ? (uint32_t*)x_len + co : d_chunk_lens;
        hash_k[k] = k ? (uint64_t*)x_hash + co : d_chunk_hashes;
        first_k[k] = k ? (uint32_t*)x_first + po : d_part_first;
        co += k ? pk->chunk_cap + 1 : 0;
        po += k ? (uint64_t)pk->nparts + 1 : 0;
        if ((err = chunk_scan(ctx, pk, d_data, sb)))
            break;
        hipEvent_t scanned = lthip_sync_event(ctx);
        hipError_t e = hipEventRecord(scanned, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamWaitEvent(c2->stream, scanned, 0);
        if (e != hipSuccess)
            err = lthip_fail(ctx, EIO, "lthip_chunk_hash (the wait of the second stream for a scan)", hipGetErrorString(e));
        else if ((err = chunk_cut_hash(c2, pk, d_data, sb, offs_k[k], lens_k[k], hash_k[k], first_k[k])))
            (void)lthip_fail(ctx, err, "lthip_chunk_hash (a slice on the second stream)", c2->err);
        if (bitmaps)
        {
            sb.bm0 += pk->bm0_words;
            sb.bm1 += pk->bm1_words;
        }
        sb.region += pk->chunk_cap;
        sb.part_count += pk->nparts;
        if (sb.cv_runs)
            sb.cv_runs += lthip_plan_run_slots(pk) * 8;
    }
    // the join (also after a failure: the context's stream never runs ahead of the second one)
    hipEvent_t hashed = lthip_sync_event(ctx);
    hipError_t e = hipEventRecord(hashed, c2->stream);
    if (e == hipSuccess)
        e = hipStreamWaitEvent(ctx->stream, hashed, 0);
    if (e != hipSuccess)
    {
        (void)hipStreamSynchronize(c2->stream);
        if (!err)
            err = lthip_fail(ctx, EIO, "lthip_chunk_hash (the join of the second stream)", hipGetErrorString(e));
    }
    if (!err)
    {
        LaunchTimer t(ctx, LTHIP_K_COMPACT);
        for (uint32_t k = 1; k < S; ++k) // in order: slice k's base is the total behind slice k - 1's join
        {
            const lthip_plan* pk = plan->slice[k];
            const uint64_t n = pk->chunk_cap > (uint64_t)pk->nparts + 1 ? pk->chunk_cap : (uint64_t)pk->nparts + 1;
            hipLaunchKernelGGL(k_slice_join, dim3((uint32_t)div_up_u64(n, 256)), dim3(256), 0, ctx->stream, (const uint64_t*)offs_k[k], (const uint32_t*)lens_k[k],
                               (const uint64_t*)hash_k[k], (const uint32_t*)first_k[k], pk->nparts, d_part_first + plan->slice_first[k], d_chunk_offsets,
                               d_chunk_lens, d_chunk_hashes);
        }
        if ((e = hipGetLastError()) != hipSuccess)
            err = lthip_fail(ctx, EIO, "kernel launch", hipGetErrorString(e));
    }
    return err;
}

extern "C" int lthip_chunk_hash(lthip_ctx* ctx, const lthip_plan* plan, const void* d_data, uint64_t* d_chunk_offsets,
                                uint32_t* d_chunk_lens, uint64_t* d_chunk_hashes, uint32_t* d_part_first,
                                uint64_t* out_total)
{
    if (!ctx || !plan || !d_chunk_offsets || !d_chunk_lens || !d_part_first || (plan->total_bytes && !d_data))
        return EINVAL;
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    bool sliced;
    int err = chunk_hash_sliced(ctx, plan, d_data, d_chunk_offsets, d_chunk_lens, d_chunk_hashes, d_part_first, &sliced);
    ScanBuffers sb;
    if (!sliced && !(err = chunk_scan_buffers(ctx, plan, !plan_walks(plan), d_chunk_hashes != nullptr, &sb)) && !(err = chunk_scan(ctx, plan, d_data, sb)))
        err = chunk_cut_hash(ctx, plan, d_data, sb, d_chunk_offsets, d_chunk_lens, d_chunk_hashes, d_part_first);
    if (err)
        return err;
    if (out_total)
    {
        uint32_t total = 0;
        LTHIP_CHECK(ctx, hipMemcpyAsync(&total, d_part_first + plan->nparts, 4, hipMemcpyDeviceToHost, ctx->stream));
        LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
        *out_total = total;
    }
    return 0;
}

extern "C" int lthip_chunk_from_buffer(lthip_ctx* ctx, const void* d_data, uint64_t size, uint32_t min_chunk,
                                       uint32_t avg_chunk, uint32_t max_chunk, uint64_t* out_len)
{
    if (!ctx || !d_data || !out_len || size == 0)
        return EINVAL;
    if (min_chunk < 48 || min_chunk > avg_chunk || avg_chunk > max_chunk)
        return lthip_fail(ctx, EINVAL, "lthip_chunk_from_buffer", "need 48 <= min <= avg <= max");
    if (size <= min_chunk)
    {
        *out_len = size; // hpcdcchunker.c:479-484
        return 0;
    }
    const uint32_t d = discriminator_from_avg(avg_chunk);
    if (d == 0)
        return lthip_fail(ctx, EINVAL, "lthip_chunk_from_buffer", "discriminator is zero");
    LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
    void* d_out;
    int err = lthip_scratch(ctx, S_MISC, 64, &d_out);
    if (err)
        return err;
    const uint32_t n = (uint32_t)(size > max_chunk ? max_chunk : size);
    if ((err = lthip_launch_from_buffer(ctx, (const uint8_t*)d_data, n, min_chunk, make_div_test(d), (uint64_t*)d_out)))
        return err;
    uint64_t len = 0;
    LTHIP_CHECK(ctx, hipMemcpyAsync(&len, d_out, 8, hipMemcpyDeviceToHost, ctx->stream));
    LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
    *out_len = len;
    return 0;
}
