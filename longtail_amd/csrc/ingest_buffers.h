// ingest_buffers.h -- the workspaces of the ingest sessions (ingest.hip, ingest_stream.hip): device and pinned buffers that are grown
// when a call needs more and kept otherwise, so that a session allocates nothing in steady state; and the sessions' rule from a block's
// tag to its codec (include/longtail_hip.h, TAGS AND CODECS).  Included into both translation units.
#pragma once
#include "lthip_internal.h"

namespace
{

struct DBuf
{
    void* p = nullptr;
    size_t cap = 0;
};
struct HBuf
{
    void* p = nullptr;
    size_t cap = 0;
};

int reserve_dev(lthip_ctx* ctx, DBuf& b, size_t bytes)
{
    if (bytes == 0)
        bytes = 256;
    if (b.cap >= bytes)
        return 0;
    if (b.p)
    {
        LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
        LTHIP_CHECK(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t cap = bytes + bytes / 8 + 4096;
    LTHIP_CHECK(ctx, lthip_hip_malloc(&b.p, cap));
    b.cap = cap;
    return 0;
}

int reserve_pinned(lthip_ctx* ctx, HBuf& b, size_t bytes)
{
    if (bytes == 0)
        bytes = 256;
    if (b.cap >= bytes)
        return 0;
    if (b.p)
    {
        LTHIP_CHECK(ctx, lthip_stream_wait(ctx));
        LTHIP_CHECK(ctx, hipHostFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    const size_t cap = bytes + bytes / 8 + 4096;
    LTHIP_CHECK(ctx, lthip_hip_host_malloc(&b.p, cap, hipHostMallocDefault));
    b.cap = cap;
    return 0;
}

// ---- which codec writes a block (enum lthip_codec of the session x the block's tag) ----
constexpr uint32_t LTHIP_TAG_LZ4 = 0x6C7A3432u; // 'lz42', lib/lz4/longtail_lz4.c:10

// LTHIP_CODEC_NONE / _LZ4 / _ZSTD for a tag LTHIP_CODEC_BY_TAG writes, -1 for every other tag (compressblockstore.c:85-97 picks the
// codec from the registry by the tag; 0 is stored as it is)
int codec_of_tag(uint32_t tag)
{
    if (tag == 0u)
        return LTHIP_CODEC_NONE;
    if (tag == LTHIP_TAG_LZ4)
        return LTHIP_CODEC_LZ4;
    if ((tag >> 8) == 0x7A7464u /* 'ztd' */ && (tag & 0xFFu) >= '1' && (tag & 0xFFu) <= '5')
        return LTHIP_CODEC_ZSTD;
    return -1;
}

// 0 when a session of `codec` takes the tag; EINVAL: LTHIP_CODEC_NONE and a tag other than 0; ENOTSUP: LTHIP_CODEC_BY_TAG and a tag that
// names no codec of this library.  LZ4 / ZSTD take any tag (the caller vouches for them).
int tag_refusal(uint32_t codec, uint32_t tag)
{
    if (codec == LTHIP_CODEC_NONE)
        return tag == 0u ? 0 : EINVAL;
    if (codec == LTHIP_CODEC_BY_TAG)
        return codec_of_tag(tag) < 0 ? ENOTSUP : 0;
    return 0;
}

// the codec of one block and, for zstd, the parse: one key per codec call
struct BlockCodec
{
    uint32_t codec;
    int quality;
    bool operator==(const BlockCodec& o) const { return codec == o.codec && quality == o.quality; }
};
BlockCodec block_codec(const lthip_ingest_config& cfg, uint32_t tag)
{
    BlockCodec c = {cfg.codec, 0};
    if (cfg.codec == LTHIP_CODEC_BY_TAG)
        c.codec = (uint32_t)codec_of_tag(tag); // (refused up front: never -1 here)
    if (c.codec == LTHIP_CODEC_ZSTD) // ('ztd4': high, 'ztd3' / 'ztd5': max)
        c.quality = lthip_zstd_quality_of_settings(cfg.codec == LTHIP_CODEC_BY_TAG ? tag : cfg.compression_type);
    return c;
}
size_t block_codec_bound(uint32_t codec, size_t n) { return codec == LTHIP_CODEC_LZ4 ? lthip_lz4_bound(n) : codec == LTHIP_CODEC_ZSTD ? lthip_zstd_bound(n) : n; }
// the bytes in front of a block's payload: BlockIndex, and the [raw][compressed] words unless the block is stored raw
size_t block_header_bytes(uint32_t codec, uint32_t chunks) { return codec == LTHIP_CODEC_NONE ? lthip_block_index_size(chunks) : lthip_stored_block_header_size(chunks); }

} // namespace
