// lz4_grid_rule.h -- the launch grid of k_lz4_segments (k_lz4.hip).  Host only, plain C++: tests/test_lz4_grid_rule.py compiles it
// without HIP.
//
// A workgroup of k_lz4_segments owns one window group of one block.  Two ways to tell a workgroup which:
//   (a) a two-dimensional grid: blockIdx.y is the block, blockIdx.x the group inside it.  The grid is as wide as the batch's LONGEST
//       block; a workgroup whose x lies beyond its own block's groups returns at once.  Nothing is searched.
//   (b) a one-dimensional grid over the batch's groups: every workgroup bisects the block table for its group (ten dependent
//       loads at 900 blocks, before its first data load).
// (a) pays with workgroups that start only to leave, so it is taken when they are few -- at most a quarter on top of the real ones --
// and the grid fits the launch limits; (b) otherwise (one 8 MiB block beside thousands of tiny ones: (a) would start hundreds of
// workgroups per tiny block).
#pragma once
#include <stdint.h>

struct Lz4Grid
{
    uint32_t x, y;
    bool two_d; // form (a)
};

constexpr uint64_t LZ4_GRID_MAX_X = 0x7FFFFFFFull; // gridDim.x
constexpr uint64_t LZ4_GRID_MAX_Y = 65535ull;      // gridDim.y
constexpr uint64_t LZ4_GRID_MAX_THREADS = 0xFFFFFFFFull; // threads of one launch (HIP refuses more)

// total_groups = the sum of the blocks' group counts (below 2^31: upload_blocks refuses more units than that), max_groups = the largest
// of them, threads = threads of a workgroup
inline Lz4Grid lz4_grid_rule(uint64_t total_groups, uint32_t max_groups, uint32_t block_count, uint32_t threads)
{
    const uint64_t cells = (uint64_t)max_groups * block_count;
    const bool fits = max_groups <= LZ4_GRID_MAX_X && block_count <= LZ4_GRID_MAX_Y && cells * threads <= LZ4_GRID_MAX_THREADS;
    if (total_groups != 0 && fits && 4u * cells <= 5u * total_groups)
        return Lz4Grid{max_groups, block_count, true};
    return Lz4Grid{(uint32_t)total_groups, 1u, false};
}
