// ingest_buffers.h -- what the ingest sessions (ingest.hip, ingest_stream.hip) share with the block writer (block_images.hip): the
// workspaces -- device and pinned buffers that are grown when a call needs more and kept otherwise, so that a session allocates nothing
// in steady state --, the rule from a block's tag to its codec (include/longtail_hip.h, TAGS AND CODECS), and the host side of a batch
// of stored-block images: its blocks, their slots in the arena, the images a caller may fetch.  Included into the three translation units.
#pragma once
#include "lthip_internal.h"
#include "store_layout.h"

#include <utility>

// a device / pinned buffer that frees itself, and an event that destroys itself: members of the sessions and of the bulk calls' local
// workspaces, so that no destroy function lists them.  Movable, not copyable.  (The owner sets the device before they go.)
template <hipError_t (*Release)(void*)> struct OwnedBuf
{
    void* p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept // (what this one held leaves with `o`)
    {
        std::swap(p, o.p), std::swap(cap, o.cap);
        return *this;
    }
    ~OwnedBuf() { (void)release(); }
    hipError_t release()
    {
        const hipError_t e = p ? Release(p) : hipSuccess;
        p = nullptr, cap = 0;
        return e;
    }
};
typedef OwnedBuf<hipFree> DBuf;
typedef OwnedBuf<hipHostFree> HBuf;

struct Event
{
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept
    {
        std::swap(e, o.e);
        return *this;
    }
    ~Event()
    {
        if (e)
            (void)hipEventDestroy(e);
    }
    hipError_t create() { return hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    operator hipEvent_t() const { return e; }
};

// the codec of one block and, for zstd, the parse: one key per codec call
struct BlockCodec
{
    uint32_t codec;
    int quality;
    bool operator==(const BlockCodec& o) const { return codec == o.codec && quality == o.quality; }
};

// host tables of one lthip_gather_ranges call.  merge_bytes != 0: neighbours that continue each other on both sides become one range, up
// to that many bytes -- the gather kernel copies a range per workgroup, so small chunks share a workgroup and a long run still spreads
// over the device instead of being copied by one CU
struct Ranges
{
    std::vector<uint64_t> src, dst;
    std::vector<uint32_t> len;
    void clear() { src.clear(), dst.clear(), len.clear(); }
    void add(uint64_t s, uint32_t l, uint64_t d, uint64_t merge_bytes)
    {
        if (l == 0)
            return;
        if (!src.empty() && src.back() + len.back() == s && dst.back() + len.back() == d && (uint64_t)len.back() + l <= merge_bytes)
            len.back() += l;
        else
        {
            src.push_back(s);
            len.push_back(l);
            dst.push_back(d);
        }
    }
};

// the device tables the block writer grows and keeps: one set per session
struct BlockImageBufs
{
    DBuf d_tmpsz, d_gsrc, d_glen, d_gdst, d_bfirst, d_braw, d_bimg, d_btag;
};

inline size_t block_codec_bound(uint32_t codec, size_t n) { return codec == LTHIP_CODEC_LZ4 ? lthip_lz4_bound(n) : codec == LTHIP_CODEC_ZSTD ? lthip_zstd_bound(n) : n; }
// the bytes in front of a block's payload: BlockIndex, and the [raw][compressed] words unless the block is stored raw
inline size_t block_header_bytes(uint32_t codec, uint32_t chunks) { return codec == LTHIP_CODEC_NONE ? lthip_block_index_size(chunks) : lthip_stored_block_header_size(chunks); }

constexpr uint32_t PLACE_RAW = ~0u; // BlockBatch::place of a block that is copied straight from where its chunks lie
constexpr uint32_t PLACE_IN_IMAGE = ~0u - 1u; // ... of a raw block whose chunks lie in its image already (the repack session): nothing is copied

// One batch of stored-block images, as the session describes it block after block (add) and the writer lays it out: a slot of the arena
// per block -- BlockIndex, the [raw][compressed] words unless the block is stored raw, the bound of the block's own codec, rounded to
// 64 bytes -- and the distinct (codec, zstd quality) keys in the order they appear.  A session keeps one and reuses its vectors.
struct BlockBatch
{
    std::vector<uint32_t> first; // count + 1: the blocks' chunk ranges, relative to the batch's first chunk
    std::vector<uint32_t> raw, tag, hdr; // raw bytes, tag and the bytes in front of the payload
    std::vector<BlockCodec> codec, keys;
    std::vector<uint32_t> place;           // which base pointer the block's bytes lie behind (lthip_block_payloads), or PLACE_RAW
    std::vector<uint64_t> src_off, img_off; // ... and where; the image's offset in the arena
    uint64_t arena;                        // bytes of the slots so far: for the session to judge
    // (the writer's own tables, kept for their capacity)
    std::vector<uint64_t> c_src, c_dst, r_payload;
    std::vector<uint32_t> c_size, c_cap, which, r_first, r_count;
    Ranges scatter;

    size_t count() const { return raw.size(); }
    void clear()
    {
        first.assign(1, 0u);
        raw.clear(), tag.clear(), hdr.clear(), place.clear(), codec.clear(), keys.clear(), src_off.clear(), img_off.clear();
        arena = 0;
    }
    static uint64_t slot(uint32_t codec, uint32_t chunks, uint64_t raw_bytes)
    {
        return ((uint64_t)block_header_bytes(codec, chunks) + block_codec_bound(codec, raw_bytes) + 63u) & ~(uint64_t)63u;
    }
    void add(uint32_t chunks, uint64_t raw_bytes, uint32_t block_tag, BlockCodec bc, uint32_t where, uint64_t offset)
    {
        first.push_back(first.back() + chunks);
        raw.push_back((uint32_t)raw_bytes);
        tag.push_back(block_tag);
        hdr.push_back((uint32_t)block_header_bytes(bc.codec, chunks));
        codec.push_back(bc);
        if (bc.codec != LTHIP_CODEC_NONE && std::find(keys.begin(), keys.end(), bc) == keys.end())
            keys.push_back(bc);
        place.push_back(where);
        src_off.push_back(offset);
        img_off.push_back(arena);
        arena += slot(bc.codec, chunks, raw_bytes);
    }
};

// the stored-block images of the last batch, for lthip_ingest_images / lthip_ingest_stream_images: first block, offsets in the arena,
// header sizes; the image sizes are complete once the compressed sizes are on the host
struct BlockImages
{
    uint64_t first_block = 0;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> sizes, hdr; // header + payload per image: computed from hdr every time (completing twice adds nothing twice)
    void set(uint64_t b0, const BlockBatch& bt)
    {
        first_block = b0;
        offsets = bt.img_off;
        hdr = bt.hdr;
        sizes = bt.hdr; // (headers only until the payload sizes are known)
    }
    void complete(const uint32_t* comp_sizes /* of all blocks */)
    {
        for (size_t i = 0; i < hdr.size(); ++i)
            sizes[i] = hdr[i] + comp_sizes[first_block + i]; // header (BlockIndex + [raw][compressed]) + payload
    }
    void get(uint64_t* out_first_block, uint64_t* out_count, const uint64_t** out_offsets, const uint32_t** out_sizes) const
    {
        if (out_first_block)
            *out_first_block = first_block;
        if (out_count)
            *out_count = offsets.size();
        if (out_offsets)
            *out_offsets = offsets.data();
        if (out_sizes)
            *out_sizes = sizes.data();
    }
};

namespace
{

// room for `bytes` in a buffer: kept when it has them, else replaced by one an eighth larger (what it held is dropped)
template <class Buf, class Alloc> int reserve_buf(lthip_ctx* ctx, Buf& b, size_t bytes, Alloc alloc)
{
    if (bytes == 0)
        bytes = 256;
    if (b.cap >= bytes)
        return 0;
    if (b.p)
    {
        LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
        LTHIP_CHECK(ctx, b.release());
    }
    const size_t cap = bytes + bytes / 8 + 4096;
    LTHIP_CHECK(ctx, alloc(&b.p, cap));
    b.cap = cap;
    return 0;
}
int reserve_dev(lthip_ctx* ctx, DBuf& b, size_t bytes) { return reserve_buf(ctx, b, bytes, lthip_hip_malloc); }
int reserve_pinned(lthip_ctx* ctx, HBuf& b, size_t bytes)
{
    return reserve_buf(ctx, b, bytes, [](void** p, size_t n) { return lthip_hip_host_malloc(p, n, hipHostMallocDefault); });
}

// ---- which codec writes a block (enum lthip_codec of the session x the block's tag) ----
BlockCodec block_codec(const lthip_ingest_config& cfg, uint32_t tag)
{
    BlockCodec c = {cfg.codec, 0};
    if (cfg.codec == LTHIP_CODEC_BY_TAG)
        c.codec = (uint32_t)codec_of_tag(tag); // (refused up front: never -1 here)
    if (c.codec == LTHIP_CODEC_ZSTD) // ('ztd4': high, 'ztd3' / 'ztd5': max)
        c.quality = lthip_zstd_quality_of_settings(cfg.codec == LTHIP_CODEC_BY_TAG ? tag : cfg.compression_type);
    return c;
}

} // namespace
