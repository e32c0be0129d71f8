"""The launch grid of k_lz4_segments (longtail_amd/csrc/lz4/lz4_grid_rule.h), compiled for the host as it stands.  No GPU.

The rule chooses between a two-dimensional grid (y = block, x = group inside it, as wide as the longest block; a workgroup beyond its
block's groups returns at once) and the one-dimensional grid over the batch's groups (the block found by bisection).  Asserted:
  equal blocks take the two-dimensional grid, and it covers every (block, group) once: x = the groups of a block, y = the blocks
  one long block among thousands of short ones takes the one-dimensional grid, x = the batch's groups
  the two-dimensional grid is taken only while  longest block x blocks <= 1.25 x groups  -- on either side of that bound
  no block and one block are handled
  every answer stays within the launch limits, also where the two-dimensional grid would not"""
import pytest

from tests import lz4_grid_rule_host as H


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    if H.host_compiler() is None:
        pytest.skip("no host C++ compiler")
    program = H.build(tmp_path_factory.mktemp("lz4grid"))
    return lambda cases: H.ask(program, cases)


def covered(grid, groups):
    """the (block, group) pairs that the grid's workgroups take up, as k_lz4_segments reads them -> a list (duplicates kept)"""
    x, y, two_d = grid
    if two_d:
        return [(b, g) for b in range(y) for g in range(x) if g < groups[b]]
    assert y == 1
    bases, out = [0], []
    for n in groups[:-1]:
        bases.append(bases[-1] + n)
    for grp in range(x):
        b = max(i for i, base in enumerate(bases) if base <= grp)  # (what the bisection finds: the last block that starts at or before grp)
        out.append((b, grp - bases[b]))
    return out


def test_equal_blocks_take_the_two_dimensional_grid(rule):
    for blocks, size in ((900, 9 << 20), (7, 1 << 20), (64, 32768), (3, 1), (2, 40000)):
        sizes = [size] * blocks
        groups = H.groups_of(sizes)
        (grid,) = rule([H.batch_case(sizes)])
        assert grid == (groups[0], blocks, True), (blocks, size, grid)
        got = covered(grid, groups)
        assert len(got) == len(set(got)) == sum(groups) and set(got) == {(b, g) for b in range(blocks) for g in range(groups[b])}


def test_unequal_blocks_within_the_bound_are_covered_once(rule):
    sizes = [300000, 262144, 280000, 299999, 270000, 1 << 18]
    groups = H.groups_of(sizes)
    assert 4 * max(groups) * len(groups) <= 5 * sum(groups)
    (grid,) = rule([H.batch_case(sizes)])
    assert grid == (max(groups), len(sizes), True)
    got = covered(grid, groups)
    assert sorted(got) == [(b, g) for b in range(len(sizes)) for g in range(groups[b])]


def test_one_long_block_among_short_ones_takes_the_one_dimensional_grid(rule):
    for sizes in ([8 << 20] + [64] * 3000, [64] * 1500 + [1 << 20] + [64] * 1500, [100] * 4000 + [8 << 20]):
        groups = H.groups_of(sizes)
        (grid,) = rule([H.batch_case(sizes)])
        assert grid == (sum(groups), 1, False), grid
    sizes = [1 << 20] + [64] * 40  # small enough to walk
    groups = H.groups_of(sizes)
    (grid,) = rule([H.batch_case(sizes)])
    assert grid == (sum(groups), 1, False)
    assert sorted(covered(grid, groups)) == [(b, g) for b in range(len(sizes)) for g in range(groups[b])]


def test_the_bound_is_a_quarter_on_top(rule):
    # 100 blocks, the longest of 50 groups: 5000 cells; taken from 4000 groups on
    for total, two_d in ((4000, True), (3999, False), (5000, True), (50, False)):
        (grid,) = rule([(total, 50, 100, H.THREADS)])
        assert grid == ((50, 100, True) if two_d else (total, 1, False)), (total, grid)


def test_no_block_and_one_block(rule):
    none, empty_only, one, one_byte = rule([(0, 0, 0, H.THREADS), H.batch_case([0, 0]), H.batch_case([5 << 20]), H.batch_case([1])])
    assert none == (0, 1, False) and empty_only == (0, 1, False)  # (nothing to launch: the caller launches no grid of 0)
    assert one == (H.groups_of([5 << 20])[0], 1, True) and one_byte == (1, 1, True)


def test_every_answer_is_within_the_launch_limits(rule):
    cases = [(65535 * 4, 4, 65535, H.THREADS), (65536 * 4, 4, 65536, H.THREADS),          # y at and past its limit
             (2 * 4194303, 4194303, 2, H.THREADS), (2 * 4194304, 4194304, 2, H.THREADS),  # x * y * threads at and past 2^32
             (8388607, 8388607, 1, H.THREADS), (8388608, 8388608, 1, H.THREADS),
             (0x7FFFFFF0 // 8, 300, 65535, H.THREADS), (262144, 288, 911, H.THREADS), (1, 1, 1, 1024)]
    want_two_d = [True, False, True, False, True, False, False, True, True]
    for case, grid, two_d in zip(cases, rule(cases), want_two_d):
        x, y, got = grid
        assert got == two_d, (case, grid)
        assert x <= H.MAX_X and 1 <= y <= H.MAX_Y, (case, grid)
        if got:
            assert x * y * case[3] <= H.MAX_THREADS and (x, y) == (case[1], case[2]), (case, grid)
        else:
            assert (x, y) == (case[0], 1), (case, grid)
