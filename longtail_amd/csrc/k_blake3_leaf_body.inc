// The blocks of one leaf, in a lane's registers (included by k_blake3_leaves and by b3_leaf, k_blake3_leaf.h, where it stands: the
// same text in both, because the leaf kernel's 64 registers hold only for the code the allocator sees there -- called through a function,
// the same statements came out with six spilled values).
// In scope: cv[8] = the IV, q = the 4-byte aligned address at or below the leaf's first byte, mis = the bytes between (sh = 8 mis), k = the
// leaf's index in its range, llen = its bytes in nblocks blocks, root = F_ROOT for a range of one leaf.  cv <- the leaf's chaining value.
// The message dwords of block b + 1 are loaded while block b is compressed (two register sets that swap roles by name, the loop unrolled
// by two): k_blake3.hip, at the kernel.
const uint32_t last = nblocks - 1u;
const uint32_t bl = llen - last * 64u;                  // 0..64 bytes in the last block
const uint32_t nd = bl ? (mis + bl + 3u) >> 2 : 0u;    // its dwords that intersect [p, p + bl)
// Blocks 0 .. last - 2 (the block behind each is interior too) go through a loop of two halves: the first compresses wa while
// wb is in flight, the second wb while wa is.  A lane with an odd number of them sits out the first half of the first trip,
// so every lane leaves at the bottom with block last - 1 in wa, and a wave makes no more trips than its longest lane needs.
uint32_t wa[17], wb[17];
uint32_t b = 0;
bool first_half = last > 1u && ((last - 1u) & 1u) == 0u;
if (last > 1u && !first_half)
    b3_load_interior(wb, q);
else if (last)
    b3_load_interior(wa, q);
if (last > 1u)
{
#pragma unroll 1
    for (;;)
    {
        if (first_half)
        {
            b3_load_interior(wb, q + (b + 1u) * 16u);
            b3_pin(cv);
            b3_interior_block(cv, wa, sh, k, b == 0 ? (uint32_t)F_CHUNK_START : 0u);
            b3_pin(cv);
            ++b;
        }
        first_half = true;
        b3_load_interior(wa, q + (b + 1u) * 16u);
        b3_pin(cv);
        b3_interior_block(cv, wb, sh, k, b == 0 ? (uint32_t)F_CHUNK_START : 0u);
        b3_pin(cv);
        ++b;
        if (b + 1u >= last)
            break;
    }
}
// block last - 1 is loaded, the last interior one: the last block's dwords are asked for before it is compressed
if (last)
{
    b3_load_last(wb, q + last * 16u, nd);
    b3_pin(cv);
    b3_interior_block(cv, wa, sh, k, b == 0 ? (uint32_t)F_CHUNK_START : 0u);
    b3_pin(cv);
}
else
    b3_load_last(wb, q, nd);
b3_last_block(cv, wb, sh, k, bl, (uint32_t)F_CHUNK_END | root | (last == 0 ? (uint32_t)F_CHUNK_START : 0u));
