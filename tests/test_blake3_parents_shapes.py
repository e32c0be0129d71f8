"""The shape arithmetic of the small-tree parents kernel (k_blake3.hip, between the marks `[b3-parents-shapes` .. `b3-parents-shapes]`),
compiled for the host as it stands and walked for every range of n = 1 .. 256 leaves and every block size B = 2^J that was built
(J = 1, 2, 3).  No GPU.

The walker below repeats the kernel's loops and nothing else: the register stage of every block (for st, for k, b3s_reg_merge), then
the LDS levels from a list that each level filters for the next (b3s_lds_merge).  Asserted for every (J, n):
  the merges are exactly those of the left-heavy tree, the pairs (k, k + st) with st a power of two, k = 0 mod 2 st, k + st < n
  each occurs once, and after the merges that made its two children
  ROOT is on the last merge and on no other; a range of one leaf has no merge and does not go to LDS
  a range's share of the LDS array (table entries and nodes) is within the bound per leaf slot that sizes the array"""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "longtail_amd" / "csrc" / "k_blake3.hip"
JS = (1, 2, 3)

WALKER = r"""
#include <stdint.h>
#include <stdio.h>
#include <vector>
@SHAPES@
int main()
{
    for (uint32_t J = 1; J <= 3; ++J)
    {
        const uint32_t B = 1u << J;
        for (uint32_t n = 1; n <= 256; ++n)
        {
            const uint32_t nb = b3s_blocks(n, B);
            printf("range %u %u lds %d blocks %u bytes %u\n", J, n, (int)b3s_to_lds(n, B), nb, b3s_range_bytes(n, B));
            for (uint32_t b = 0; b < nb; ++b) // register stage: a thread per block
            {
                const uint32_t m = b3s_block_leaves(n, b, B);
                printf("block %u %u\n", b * B, m);
                for (uint32_t st = 1; st < B; st <<= 1)
                    for (uint32_t k = 0; k + st < B; k += 2u * st)
                        if (b3s_reg_merge(m, k, st))
                            printf("merge %u %u %d\n", b * B + k, st, (int)b3s_root(n, b * B + k, st));
            }
            if (!b3s_to_lds(n, B))
                continue;
            std::vector<uint32_t> list, next; // LDS levels: the first list is made by the register stage
            for (uint32_t b = 0; b < nb; ++b)
                if (b3s_lds_merge(nb, b, 1u))
                    list.push_back(b);
            for (uint32_t st = 1; !list.empty(); st <<= 1)
            {
                next.clear();
                for (uint32_t k : list)
                {
                    printf("merge %u %u %d\n", k * B, st * B, (int)b3s_lds_root(nb, st));
                    if (b3s_lds_merge(nb, k, 2u * st))
                        next.push_back(k);
                }
                list.swap(next);
            }
        }
    }
    for (uint32_t J = 1; J <= 3; ++J)
        for (uint32_t S = 1; S <= 4400; S += 7)
            printf("bound %u %u %u %u\n", J, S, b3s_max_nodes(S, 1u << J), b3s_max_bytes(S, 1u << J));
    return 0;
}
"""


def host_compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    return None


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """{(J, n): {"lds", "blocks", "bytes", "leaves": [(first leaf, count)], "merges": [(k, st, root)]}}, bounds [(J, S, nodes, bytes)]"""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    text = SRC.read_text()
    section = re.search(r"// \[b3-parents-shapes\n(.*?)// b3-parents-shapes\]", text, re.S).group(1)
    d = tmp_path_factory.mktemp("b3s")
    (d / "walk.cpp").write_text(WALKER.replace("@SHAPES@", section))
    res = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-o", str(d / "walk"), str(d / "walk.cpp")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    out = subprocess.run([str(d / "walk")], capture_output=True, text=True, check=True).stdout
    ranges, bounds, cur = {}, [], None
    for line in out.splitlines():
        f = line.split()
        if f[0] == "range":
            cur = ranges[(int(f[1]), int(f[2]))] = {"lds": int(f[4]), "blocks": int(f[6]), "bytes": int(f[8]), "leaves": [], "merges": []}
        elif f[0] == "block":
            cur["leaves"].append((int(f[1]), int(f[2])))
        elif f[0] == "merge":
            cur["merges"].append((int(f[1]), int(f[2]), int(f[3])))
        else:
            bounds.append(tuple(int(x) for x in f[1:]))
    return ranges, bounds


def tree_merges(n):
    out, st = set(), 1
    while st < n:
        out |= {(k, st) for k in range(0, n, 2 * st) if k + st < n}
        st *= 2
    return out


def test_every_range_is_walked(walk):
    assert set(walk[0]) == {(J, n) for J in JS for n in range(1, 257)}


def test_blocks_hold_every_leaf_once(walk):
    for (J, n), r in walk[0].items():
        B = 1 << J
        assert r["leaves"] == [(k, min(B, n - k)) for k in range(0, n, B)], (J, n)
        assert r["blocks"] == len(r["leaves"]) and r["lds"] == (r["blocks"] > 1), (J, n)


def test_merges_are_the_left_heavy_trees(walk):
    for (J, n), r in walk[0].items():
        pairs = [(k, st) for k, st, _ in r["merges"]]
        assert len(pairs) == len(set(pairs)), f"J={J} n={n}: a merge occurs twice"
        assert set(pairs) == tree_merges(n), f"J={J} n={n}: {sorted(set(pairs) ^ tree_merges(n))}"


def test_children_come_before_parents(walk):
    for (J, n), r in walk[0].items():
        at = {(k, st): i for i, (k, st, _) in enumerate(r["merges"])}
        for (k, st), i in at.items():
            # the left child is the node (k, st / 2); the right child, over [k + st, min(k + 2 st, n)), is made by (k + st, s) for s < st
            needs = [(k, st // 2)] if st > 1 else []
            needs += [(k + st, s) for s in (1 << e for e in range(8)) if s < st and k + st + s < n]
            for c in needs:
                assert at[c] < i, f"J={J} n={n}: merge {(k, st)} before its child {c}"


def test_root_is_on_the_last_merge_only(walk):
    for (J, n), r in walk[0].items():
        roots = [i for i, (_, _, root) in enumerate(r["merges"]) if root]
        if n == 1:
            assert r["merges"] == [] and not r["lds"], (J, n)  # the leaf's own value carries ROOT and is the digest
        else:
            assert roots == [len(r["merges"]) - 1], f"J={J} n={n}: ROOT on merges {roots} of {len(r['merges'])}"
            k, st, _ = r["merges"][-1]
            assert k == 0 and st < n <= 2 * st, (J, n, k, st)


def test_lds_bound_holds_for_any_window(walk):
    """A range of n leaves takes b3s_range_bytes(n) of the array; per leaf slot that is at most c = max(6, 70 / (B + 1)), so any ranges
    of S slots in all take at most c S, plus the tables' closing entry (6) and the nodes' alignment (< 16): b3s_max_bytes(S)."""
    ranges, bounds = walk
    for (J, n), r in ranges.items():
        B = 1 << J
        assert r["bytes"] == 6 + (32 * r["blocks"] if r["lds"] else 0), (J, n)
        assert r["bytes"] * (B + 1) <= max(6 * (B + 1), 70) * n, (J, n)
        assert (r["blocks"] if r["lds"] else 0) * (B + 1) <= 2 * n, (J, n)
    assert bounds
    for J, S, nodes, nbytes in bounds:
        B = 1 << J
        assert nodes == 2 * S // (B + 1) and nbytes >= max(6 * (B + 1), 70) * S // (B + 1) + 6 + 15, (J, S)
