// store_layout.h -- what a store looks like, on the host and without a line of HIP: Longtail_CreateStoreIndex's greedy packing rule, the
// tables a block-hash launch takes, the serialized StoreIndex, the caller's lthip_ingest_result and which tags a session's codec mode
// takes.  Shared by the ingest sessions (ingest.hip, ingest_stream.hip), the bulk calls (version_index.hip, k_gather.hip) and restore_call.h.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/longtail_hip.h"

namespace
{

// ---- packing (Longtail_CreateStoreIndex, src/longtail.c:6801-6860) ----
uint64_t block_limit(uint32_t max_block_size) { return (uint64_t)max_block_size + max_block_size / 10; }

// The end of the block that starts at chunk i of the n chunks seen so far: chunks of one tag (tags == null: the list has one tag), at most
// max_chunks of them, at most `limit` bytes.  *size = the block's bytes.  Whether a block that ends at n is closed is the caller's rule.
template <class Index>
Index next_block_end(const uint32_t* lens, const uint32_t* tags, Index i, Index n, uint64_t max_chunks, uint64_t limit, uint64_t* size)
{
    uint64_t s = lens[i];
    Index j = i + 1;
    while (j < n && j - i < max_chunks && (!tags || tags[j] == tags[i]) && s + lens[j] <= limit)
        s += lens[j++];
    *size = s;
    return j;
}

// ---- block hashes = the hash of each block's chunk-hash array (:3753-3757): the ranges of lthip_hash_ranges_by_id over the 8-byte
// hashes of the chunk list, with what the launcher would otherwise read back ----
struct BlockHashRanges
{
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    uint32_t max_len;
    uint64_t leaves; // 1 KiB leaves of all ranges

    // first[0 .. nb]: where every block starts in the chunk list, `base` = the chunk the device list starts with
    template <class Index> void fill(const Index* first, size_t nb, uint64_t base)
    {
        off.resize(nb);
        len.resize(nb);
        max_len = 0;
        leaves = 0;
        for (size_t b = 0; b < nb; ++b)
        {
            off[b] = ((uint64_t)first[b] - base) * 8u;
            len[b] = (uint32_t)(first[b + 1] - first[b]) * 8u;
            max_len = std::max(max_len, len[b]);
            leaves += len[b] ? (len[b] + 1023u) >> 10 : 1u;
        }
    }
};

// ---- the serialized StoreIndex (Longtail_CreateStoreIndexFromBlocks :9060-9125, layout :8913-8931) ----
size_t store_index_size(size_t nb, size_t m) { return 16 + nb * 8 + m * 8 + nb * 12 + m * 4; } // Longtail_GetStoreIndexDataSize

// nb blocks over m chunks into `out` (store_index_size bytes); block b holds chunks [first[b], first[b + 1]).  Nothing to store:
// Longtail_CreateMissingContent returns Longtail_CreateStoreIndexFromBlocks(0, 0), hash identifier 0 (:6931-6943)
template <class Index>
void write_store_index(void* out, uint32_t hash_identifier, size_t nb, size_t m, const void* block_hashes, const void* chunk_hashes,
                       const Index* first, const uint32_t* block_tags, const void* chunk_sizes)
{
    uint8_t* w = (uint8_t*)out;
    const uint32_t head[4] = {(1u << 24) /* LONGTAIL_STORE_INDEX_VERSION_1_0_0, :19-23 */, m ? hash_identifier : 0u, (uint32_t)nb, (uint32_t)m};
    memcpy(w, head, 16);
    w += 16;
    memcpy(w, block_hashes, nb * 8); // m_BlockHashes
    w += nb * 8;
    memcpy(w, chunk_hashes, m * 8); // m_ChunkHashes
    w += m * 8;
    uint32_t* bo = (uint32_t*)w; // m_BlockChunksOffsets, m_BlockChunkCounts, m_BlockTags
    for (size_t b = 0; b < nb; ++b)
    {
        bo[b] = (uint32_t)first[b];
        bo[nb + b] = (uint32_t)(first[b + 1] - first[b]);
        bo[2 * nb + b] = block_tags[b];
    }
    w += nb * 12;
    memcpy(w, chunk_sizes, m * 4); // m_ChunkSizes
}

// ---- lthip_ingest_result: the caller says how large ITS struct is, so a header older or newer than this library's never gets written
// past its end ----
bool result_struct_ok(const lthip_ingest_result* out) { return !out || (out->struct_size >= 16 && out->struct_size <= 4096); }
constexpr const char* RESULT_STRUCT_TEXT = "out_result->struct_size must be set to sizeof(lthip_ingest_result)";
void deliver_result(lthip_ingest_result* out, lthip_ingest_result* res)
{
    if (!out)
        return;
    const uint64_t have = out->struct_size;
    res->struct_size = have < sizeof *res ? have : sizeof *res;
    memcpy(out, res, (size_t)res->struct_size);
}

// ---- tags and codecs (include/longtail_hip.h, TAGS AND CODECS) ----
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
const char* tag_refusal_text(int refused)
{
    return refused == EINVAL ? "LTHIP_CODEC_NONE writes tag 0 only" : "LTHIP_CODEC_BY_TAG: a tag names no codec of this library";
}

} // namespace
