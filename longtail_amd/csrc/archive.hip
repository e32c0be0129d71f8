// archive.hip -- one-file archives (include/longtail_hip.h, "one-file archives"): the device side of golongtail's pack, and the C
// interface of the index format.  The index is host code (archive_layout.h); the one kernel here, k_archive_pack, lays the stored-block
// images an ingest session left in its arena back to back, at whatever byte positions that gives them, which is how they lie in the body
// of an archive (lib/archiveblockstore/longtail_archiveblockstore.c:36-101).  The way back is the restore session's
// (restore.hip: lthip_restore_archive_blocks).
#include "archive_layout.h"
#include "k_copy.h"
#include "lthip_internal.h"

#include <memory>
#include <new>

namespace
{

constexpr int AT = 256;
constexpr uint32_t PACK_PIECE = 1u << 18; // bytes a workgroup copies (k_restore_cache_copy's piece)

struct PackItem
{
    uint64_t src, dst; // offsets into the arena and into d_dst
    uint32_t size, pad;
};

// grid: the call's images x pieces of PACK_PIECE bytes.  lthip_wg_copy writes exactly [dst, dst + n) and reads no dword that holds no
// byte of [src, src + n): nothing is written at or beyond the end of the call's last image, and an image may end at the last byte of
// the arena.
__global__ __launch_bounds__(AT) void k_archive_pack(const PackItem* __restrict__ items, const uint8_t* __restrict__ arena, uint8_t* __restrict__ dst)
{
    const PackItem it = items[blockIdx.x];
    const uint64_t at = (uint64_t)blockIdx.y * PACK_PIECE;
    if (at >= it.size)
        return;
    const uint32_t n = std::min<uint32_t>(PACK_PIECE, it.size - (uint32_t)at);
    lthip_wg_copy<AT>(dst + it.dst + at, arena + it.src + at, n, threadIdx.x);
}

} // namespace

struct lthip_archive_writer
{
    lthip_ctx* ctx = nullptr;
    uint64_t cursor = 0; // bytes of body appended so far
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> sizes;
    std::vector<PackItem> items; // of one append call, kept for its capacity
};

// ---- the index, host only ----
extern "C" int lthip_archive_index_size(const void* store_index, size_t si_size, const void* version_index, size_t vi_size, uint64_t* out_bytes)
{
    if (!store_index || !version_index || !out_bytes)
        return EINVAL;
    return archive_layout::index_size(store_index, si_size, version_index, vi_size, out_bytes);
}

extern "C" int lthip_archive_write_index(const void* store_index, size_t si_size, const void* version_index, size_t vi_size,
                                         const uint64_t* block_offsets, const uint32_t* block_sizes, void* out, size_t capacity)
{
    if (!store_index || !version_index || !out)
        return EINVAL;
    return archive_layout::write_index(store_index, si_size, version_index, vi_size, block_offsets, block_sizes, out, capacity);
}

extern "C" int lthip_archive_peek(const void* first_8_bytes, uint64_t* index_bytes) { return archive_layout::peek(first_8_bytes, index_bytes); }

extern "C" int lthip_archive_open(const void* index, size_t index_bytes, uint64_t body_bytes, lthip_archive** out)
{
    if (out)
        *out = nullptr;
    if (!index || !out)
        return EINVAL;
    return lthip_guarded(nullptr, nullptr, [&] {
        std::unique_ptr<lthip_archive> a(new lthip_archive()); // (freed when open refuses or runs out of memory)
        const int err = archive_layout::open(index, index_bytes, body_bytes, &a->a);
        if (!err)
            *out = a.release();
        return err;
    });
}

extern "C" void lthip_archive_close(lthip_archive* a) { delete a; }

extern "C" const void* lthip_archive_store_index(const lthip_archive* a, size_t* size)
{
    if (!a)
        return nullptr;
    if (size)
        *size = (size_t)a->a.si_bytes;
    return a->a.index.data() + a->a.si_at;
}

extern "C" const void* lthip_archive_version_index(const lthip_archive* a, size_t* size)
{
    if (!a)
        return nullptr;
    if (size)
        *size = (size_t)a->a.vi_bytes;
    return a->a.index.data() + a->a.vi_at;
}

extern "C" uint32_t lthip_archive_block_count(const lthip_archive* a) { return a ? (uint32_t)a->a.offsets.size() : 0u; }
extern "C" const uint64_t* lthip_archive_block_offsets(const lthip_archive* a) { return a ? a->a.offsets.data() : nullptr; }
extern "C" const uint32_t* lthip_archive_block_sizes(const lthip_archive* a) { return a ? a->a.sizes.data() : nullptr; }
extern "C" uint64_t lthip_archive_body_bytes(const lthip_archive* a) { return a ? a->a.body_bytes : 0u; }

// ---- the writer ----
extern "C" int lthip_archive_writer_create(lthip_ctx* ctx, lthip_archive_writer** out)
{
    if (out)
        *out = nullptr;
    if (!ctx || !out)
        return EINVAL;
    lthip_archive_writer* w = new (std::nothrow) lthip_archive_writer();
    if (!w)
        return ENOMEM;
    w->ctx = ctx;
    *out = w;
    return 0;
}

extern "C" void lthip_archive_writer_destroy(lthip_archive_writer* w) { delete w; }

static int writer_append(lthip_archive_writer* w, const void* d_arena, uint32_t count, const uint64_t* image_offsets, const uint32_t* image_sizes,
                         void* d_dst, uint64_t total, uint32_t largest)
{
    lthip_ctx* ctx = w->ctx;
    w->items.clear();
    uint64_t at = 0;
    for (uint32_t i = 0; i < count; ++i)
    {
        w->items.push_back(PackItem{image_offsets[i], at, image_sizes[i], 0u});
        at += image_sizes[i];
    }
    if (total)
    {
        LTHIP_CHECK(ctx, hipSetDevice(ctx->device));
        void* d_items = nullptr;
        int err;
        constexpr size_t PIECE = 4u << 20; // (no staging slot grows to the size of a table)
        const size_t bytes = (size_t)count * sizeof(PackItem);
        if ((err = lthip_scratch(ctx, S_ARCHIVE_ITEMS, bytes, &d_items)))
            return err;
        for (size_t o = 0; o < bytes; o += PIECE)
            if ((err = lthip_stage_upload(ctx, (uint8_t*)d_items + o, (const uint8_t*)w->items.data() + o, std::min(PIECE, bytes - o), ctx->stream)))
                return err;
        LaunchTimer tm(ctx, LTHIP_K_GATHER);
        hipLaunchKernelGGL(k_archive_pack, dim3(count, (largest + PACK_PIECE - 1u) / PACK_PIECE), dim3(AT), 0, ctx->stream, (const PackItem*)d_items,
                           (const uint8_t*)d_arena, (uint8_t*)d_dst);
        LTHIP_LAUNCH_CHECK(ctx);
    }
    // the call is queued: its blocks join the tables
    for (uint32_t i = 0; i < count; ++i)
    {
        w->offsets.push_back(w->cursor + w->items[i].dst);
        w->sizes.push_back(image_sizes[i]);
    }
    w->cursor += total;
    return 0;
}

extern "C" int lthip_archive_writer_append(lthip_archive_writer* w, const void* d_arena, uint32_t count, const uint64_t* image_offsets,
                                           const uint32_t* image_sizes, void* d_dst, uint64_t dst_capacity, uint64_t* bytes_written)
{
    if (!w || !bytes_written || (count && (!image_offsets || !image_sizes)))
        return EINVAL;
    lthip_ctx* ctx = w->ctx;
    // ---- the refusals, before anything is queued or changed ----
    uint64_t total = 0;
    uint32_t largest = 0;
    for (uint32_t i = 0; i < count; ++i)
    {
        total += image_sizes[i];
        largest = std::max(largest, image_sizes[i]);
    }
    if (total > dst_capacity)
        return lthip_fail(ctx, ENOMEM, "lthip_archive_writer_append", "the call's images exceed dst_capacity");
    if (total && (!d_arena || !d_dst))
        return lthip_fail(ctx, EINVAL, "lthip_archive_writer_append", "null arena or destination");
    if (count > 0x7FFFFFFFu || w->cursor + total < w->cursor)
        return lthip_fail(ctx, EINVAL, "lthip_archive_writer_append", "more than 2^31 - 1 images in a call");
    const int err = lthip_guarded(ctx, "lthip_archive_writer_append",
                                  [&] { return writer_append(w, d_arena, count, image_offsets, image_sizes, d_dst, total, largest); });
    if (!err)
        *bytes_written = total;
    return err;
}

extern "C" int lthip_archive_writer_blocks(const lthip_archive_writer* w, uint64_t* block_count, const uint64_t** offsets, const uint32_t** sizes,
                                           uint64_t* body_bytes)
{
    if (!w)
        return EINVAL;
    if (block_count)
        *block_count = w->offsets.size();
    if (offsets)
        *offsets = w->offsets.data();
    if (sizes)
        *sizes = w->sizes.data();
    if (body_bytes)
        *body_bytes = w->cursor;
    return 0;
}

extern "C" int lthip_archive_writer_finish(lthip_archive_writer* w, const void* store_index, size_t si_size, const void* version_index, size_t vi_size,
                                           void* h_index, size_t capacity, uint64_t* index_bytes)
{
    if (!w || !store_index || !version_index || !index_bytes)
        return EINVAL;
    lthip_ctx* ctx = w->ctx;
    uint64_t bytes = 0;
    restore_parse::StoreIndex s;
    const int err = archive_layout::index_size(store_index, si_size, version_index, vi_size, &bytes, &s);
    if (err)
        return lthip_fail(ctx, err, "lthip_archive_writer_finish", err == EBADF ? "malformed store index or version index" : "the index does not fit 32 bits");
    if (w->offsets.size() != s.block_count)
        return lthip_fail(ctx, EINVAL, "lthip_archive_writer_finish", "the appended blocks are not the store index's block count");
    for (uint32_t b = 0; b < s.block_count; ++b)
        if (w->sizes[b] < archive_layout::block_header_bytes(s.block_chunk_counts[b], s.block_tags[b]))
            return lthip_fail(ctx, EINVAL, "lthip_archive_writer_finish", "an appended image is smaller than its block's header");
    *index_bytes = bytes;
    if (!h_index || (uint64_t)capacity < bytes)
        return lthip_fail(ctx, ENOMEM, "lthip_archive_writer_finish", "the index buffer is too small: call again with *index_bytes");
    return archive_layout::write_index(store_index, si_size, version_index, vi_size, w->offsets.data(), w->sizes.data(), h_index, capacity);
}
