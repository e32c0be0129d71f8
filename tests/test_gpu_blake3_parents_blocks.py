"""-m gpu: the small-tree parents kernel of k_blake3.hip (k_blake3_parents_window: blocks of B = 2^J leaves merged in registers, their
nodes in LDS level by level) at the shapes of ITS window of W leaf slots, digest for digest against the oracle.  Equality of the
64-bit digests, no tolerance; every output word is preset to a sentinel, so a range no workgroup owns fails too.

W and B are read from the kernel's source (tests/blake3_shapes.py keeps PW = 1024 for the tables of tests/test_gpu_blake3_shapes.py,
which stay as they are).  Where this kernel can go wrong:
  straddle_s      s one-leaf ranges, a 256-leaf range, 300 one-leaf ranges: the large range ends at the window's boundary (s = W - 256),
                  starts on the window's last slot (W - 1: the window then has its most slots) or on the next window's first (W)
  totals          of exactly two windows, and of two windows and one slot
  equal ranges    of n = B - 1, B, B + 1, 2B - 1, 2B, 2B + 1, 3B + 1 leaves, enough to fill a window and start the next: ROOT inside
                  the register stage (n <= B), on the first LDS level (n <= 2B), on a carried odd node (2B + 1, 3B + 1); n = B + 1 is
                  the shape with the most nodes in LDS per slot
  a window of one-leaf ranges with every fourth one empty (the most ranges a window has), a window holding one 256-leaf range, one
  range, one empty range
The largest batch is about 2 W KiB of input."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import blake3_shapes as S
from tests.gpu_util import dev_u32, dev_u64, u64

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
_SRC = (Path(__file__).resolve().parent.parent / "longtail_amd" / "csrc" / "k_blake3.hip").read_text()
J = int(re.search(r"^constexpr uint32_t PJ = (\d+);", _SRC, re.M).group(1))
W = int(re.search(r"^constexpr int PW = (\d+);", _SRC, re.M).group(1))
B = 1 << J
EQUAL_N = (B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B + 1)


def scenarios():
    """{name: [(n, t)]}"""
    tail = lambda i: S.TAILS[i % len(S.TAILS)]
    sc = {f"straddle_{s}": S._one_leaf(s) + [(256, tail(s))] + S._one_leaf(300) for s in (W - 257, W - 256, W - 255, W - 2, W - 1, W, W + 1)}
    sc["total_two_windows"] = S._mixed(2 * W)
    sc["total_two_windows_and_one"] = S._mixed(2 * W + 1)
    for n in EQUAL_N:
        if n >= 1:
            sc[f"equal_{n}"] = [(n, tail(i)) for i in range(W // n + 3)]
    sc["one_leaf_every_fourth_empty"] = S._one_leaf(W, True)
    sc["one_256"] = [(256, 961)]
    sc["one_range"] = [(37, 961)]
    sc["one_empty_range"] = [(1, 0)]
    return sc


SCENARIOS = scenarios()


@pytest.fixture(scope="module")
def src(oracle):
    host = S.source(oracle)
    return host, torch.from_numpy(host).cuda()


def test_constants():
    assert J in (1, 2, 3) and W & (W - 1) == 0 and W >= 512, (J, W)
    for n in EQUAL_N:
        assert sum(k for k, _ in SCENARIOS[f"equal_{n}"]) > W  # the batch starts a second window
    assert max(sum(k for k, _ in v) for v in SCENARIOS.values()) <= 2 * W + 600


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_blocks_scenario(gpu, oracle, src, name):
    cases, offs, lens = S.batch(SCENARIOS[name])
    exp = oracle.blake3_many(src[0], offs, lens)
    out = torch.full((len(offs),), SENTINEL, dtype=torch.int64, device="cuda")
    gpu.hash_ranges(src[1], dev_u64(offs), dev_u32(lens), max_len=S.WINDOW_MAX_LEN, out=out)
    got = u64(out)[: len(offs)]
    assert not (msg := S.first_mismatch(got, exp, cases)), f"{name} (W={W}, B={B}): {msg}"
