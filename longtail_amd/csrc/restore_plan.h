// restore_plan.h -- the host tables a restore session's plan starts from, on the host and without a line of HIP: index arithmetic over
// restore_parse.h's reading of caller-supplied blobs, kept apart from the device code so that a sanitizer can reach it.
//   base_table           a resident base version -> per distinct chunk (hash, size, offset of its first occurrence in a resident asset)
//   store_tables         the StoreIndex -> per chunk position (hash, size, the block that holds it, its offset in that block) and per
//                        block (hash, first chunk position, chunk count, tag, raw size, 1 KiB leaves)
//   whole_asset_windows  asset_offsets -> one window per selected asset, for restore_windows::expand
// A refusal is an errno with *why set to its reason.  May throw std::bad_alloc.
// Included by restore.hip (through restore_call.h) and by the stand-alone driver tests/san/restore_plan_driver.cpp.
#pragma once
#include "restore_parse.h"
#include "restore_windows.h"

namespace restore_plan
{

constexpr uint32_t NONE = 0xFFFFFFFFu; // no position, no block
constexpr uint64_t NOWHERE = ~0ull;    // a base chunk that lies in no resident asset

struct BaseTable
{
    std::vector<uint64_t> hash, off; // per distinct chunk of the base; off: its first occurrence in a resident asset, or NOWHERE
    std::vector<uint32_t> size;
    uint32_t max_chunk = 0;
};

// asset_offsets[a]: where asset a lies in the base's base_bytes bytes, or restore_parse::SKIP (not resident).  A zero-size asset
// is accepted at any offset.
inline int base_table(const restore_parse::VersionIndex& bvi, const uint64_t* asset_offsets, uint64_t base_bytes, BaseTable* out, const char** why)
{
    const uint32_t nub = bvi.chunk_count;
    if (nub > 0x7FFFFFFFu)
        return *why = "more than 2^31 - 1 chunks in the base", EINVAL;
    std::vector<uint64_t>&uhash = out->hash, &uoff = out->off;
    std::vector<uint32_t>& usize = out->size;
    uhash.resize(nub), usize.resize(nub), uoff.assign(nub, NOWHERE);
    for (uint32_t c = 0; c < nub; ++c)
    {
        uhash[c] = bvi.chunk_hashes[c];
        usize[c] = bvi.chunk_sizes[c];
        out->max_chunk = std::max(out->max_chunk, usize[c]);
    }
    for (uint64_t a = 0; a < bvi.asset_count; ++a)
    {
        const uint64_t off = asset_offsets[a], size = bvi.asset_sizes[a];
        if (off == restore_parse::SKIP || !size)
            continue;
        if (off > base_bytes || size > base_bytes - off)
            return *why = "a resident asset's window leaves the base", EINVAL;
        const uint64_t start = bvi.asset_chunk_index_starts[a], count = bvi.asset_chunk_counts[a];
        uint64_t at = off;
        for (uint64_t k = 0; k < count; ++k)
        {
            const uint32_t c = bvi.asset_chunk_indexes[start + k];
            if (uoff[c] == NOWHERE)
                uoff[c] = at;
            at += usize[c];
        }
    }
    return 0;
}

struct StoreTables
{
    std::vector<uint64_t> chash;               // per chunk position
    std::vector<uint32_t> csize, cblock, coff; // cblock: NONE for a position no block lists
    std::vector<uint64_t> bhash, bleaves;      // per block; bleaves: the 1 KiB leaves of its chunks (an empty chunk counts one)
    std::vector<uint32_t> bcoff, bcnt, btag, braw;
    uint32_t max_chunk = 0;
    uint64_t block_chunks = 0; // the blocks' chunk counts summed: the chunk count for an index whose blocks share no chunk position
};

inline int store_tables(const restore_parse::StoreIndex& si, StoreTables* out, const char** why)
{
    const uint32_t nb = si.block_count, m = si.chunk_count;
    if (m > 0x7FFFFFFFu)
        return *why = "more than 2^31 - 1 chunks in the store index", EINVAL;
    std::vector<uint64_t>& chash = out->chash;
    std::vector<uint32_t>&csize = out->csize, &cblock = out->cblock, &coff = out->coff, &bcoff = out->bcoff;
    chash.resize(m), csize.resize(m), cblock.assign(m, NONE), coff.assign(m, 0u), bcoff.resize(nb);
    for (uint32_t c = 0; c < m; ++c)
    {
        chash[c] = si.chunk_hashes[c];
        csize[c] = si.chunk_sizes[c];
        out->max_chunk = std::max(out->max_chunk, csize[c]);
    }
    out->bhash.resize(nb), out->bcnt.resize(nb), out->btag.resize(nb), out->braw.resize(nb), out->bleaves.resize(nb);
    for (uint32_t b = 0; b < nb; ++b)
    {
        out->bhash[b] = si.block_hashes[b];
        bcoff[b] = si.block_chunk_offsets[b];
        out->bcnt[b] = si.block_chunk_counts[b];
        out->btag[b] = si.block_tags[b];
        uint64_t off = 0, leaves = 0;
        for (uint32_t k = 0; k < out->bcnt[b]; ++k)
        {
            const uint32_t c = bcoff[b] + k;
            if (cblock[c] == NONE) // (blocks that share a chunk position: no writer produces them; the first block keeps it)
            {
                cblock[c] = b;
                coff[c] = (uint32_t)off;
            }
            off += csize[c];
            leaves += csize[c] ? ((uint64_t)csize[c] + 1023u) >> 10 : 1u;
        }
        out->braw[b] = (uint32_t)off; // (below 4 GiB: parse_store_index)
        out->block_chunks += out->bcnt[b];
        out->bleaves[b] = leaves;
    }
    if (out->block_chunks > 0x7FFFFFFFull)
        return *why = "the store index's blocks list more than 2^31 - 1 chunks", EINVAL;
    return 0;
}

// a selected asset is one window of all its bytes at its offset (a directory or an empty file: a window of no bytes, whatever its offset)
inline std::vector<restore_windows::Window> whole_asset_windows(const restore_parse::VersionIndex& vi, const uint64_t* asset_offsets)
{
    std::vector<restore_windows::Window> whole;
    for (uint64_t a = 0; a < vi.asset_count; ++a)
    {
        const uint64_t off = asset_offsets[a], size = vi.asset_sizes[a];
        if (off != restore_parse::SKIP)
            whole.push_back(restore_windows::Window{(uint32_t)a, 0u, 0u, size, size ? off : 0u});
    }
    return whole;
}

} // namespace restore_plan
