"""-m gpu: lthip_hash_ranges at the edges of the leaf pass's load pipeline, digest for digest against the oracle (the one
tests/test_gpu_blake3_shapes.py uses).  Equality of the 64-bit digests, no tolerance.

k_blake3_leaves keeps the message dwords of block b + 1 in flight while it compresses block b: two register sets that swap roles, a
loop of two halves that a lane with an odd number of blocks enters in the middle, the last block's masked loads issued in front of the
last interior block's compression.  What can go wrong there is a block compressed from the wrong set, a half skipped or run twice, a
lane that has left the loop disturbed by its neighbours' loads, or a last block that misses a dword.  So:

  edges     leaves with 0, 1, 2, 3 and 15 interior blocks and the lengths around them, each at all four start residues mod 4
  ragged    about 4 000 one-leaf ranges whose neighbouring lanes differ in block count (1, 16, 2, 15, 3, 1 blocks), so the exec mask
            changes on every trip while loads are in flight
  the end   a batch whose last range ends on the last byte of the data handed to the call, the data a view inside a larger tensor

The ablation build keeps the earlier loop (every block's loads waited for in front of its compression) behind LTHIP_B3_PREFETCH=0, so
that both forms can be timed from one library; its digests are checked on the same batches.

Every output word is preset to a sentinel.  A failure names the range."""
import numpy as np
import pytest
import torch

from tests.gpu_util import dev_u32, dev_u64, u64

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
EDGE_LENS = [0, 1, 63, 64, 65, 128, 129, 192, 193, 1023, 1024, 1025, 2048 + 1, 65536]
RAGGED_LENS = [1, 1024, 65, 960, 129, 64]
RAGGED_N = 4002  # 667 turns of the cycle: 63 workgroups of 256 leaves, the last one partly filled
WINDOW_MAX_LEN = 256 * 1024  # (the call's bound of the longest range: every batch here takes the window reducer)


def edge_ranges():
    """Every length at every residue of its start address mod 4 (device allocations are 256-byte aligned and the data starts at the
    tensor's first byte, so an offset's residue is the address's)."""
    offs, lens, pos = [], [], 0
    for n in EDGE_LENS:
        for r in range(4):
            pos = (pos + 3) // 4 * 4 + r
            offs.append(pos)
            lens.append(n)
            pos += n
    return np.array(offs, np.uint64), np.array(lens, np.uint32), pos


def ragged_ranges():
    """Back to back, so the residues walk through all four as well."""
    lens = np.array([RAGGED_LENS[i % len(RAGGED_LENS)] for i in range(RAGGED_N)], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.uint64)]).astype(np.uint64)
    return offs, lens, int(lens.sum())


@pytest.fixture(scope="module")
def tables(oracle):
    """name -> (host bytes, offsets, lengths, the oracle's digests), computed once."""
    out = {}
    for name, (offs, lens, nbytes) in {"edges": edge_ranges(), "ragged": ragged_ranges()}.items():
        host = oracle.synth(nbytes, 0xB3 + len(out), 0)
        out[name] = (host, offs, lens, oracle.blake3_many(host, offs, lens))
    return out


def hash_ranges(ctx, dev, offs, lens):
    out = torch.full((len(offs),), SENTINEL, dtype=torch.int64, device="cuda")
    ctx.hash_ranges(dev, dev_u64(offs), dev_u32(lens), max_len=WINDOW_MAX_LEN, out=out)
    return u64(out)


def first_mismatch(got, exp, offs, lens):
    bad = np.flatnonzero(got != exp)
    if not len(bad):
        return ""
    i = int(bad[0])
    return (f"{len(bad)} of {len(exp)} digests differ; first: range {i} (length {int(lens[i])}, start residue {int(offs[i]) % 4}): "
            f"got {int(got[i]):016x}, expected {int(exp[i]):016x}")


def test_edge_lengths_at_every_residue(gpu, tables):
    host, offs, lens, exp = tables["edges"]
    assert sorted({(int(n), int(o) % 4) for o, n in zip(offs, lens)}) == [(n, r) for n in sorted(EDGE_LENS) for r in range(4)]
    got = hash_ranges(gpu, torch.from_numpy(host).cuda(), offs, lens)
    assert not (msg := first_mismatch(got, exp, offs, lens)), msg


def test_neighbouring_lanes_differ_in_block_count(gpu, tables):
    host, offs, lens, exp = tables["ragged"]
    assert {int(o) % 4 for o in offs} == {0, 1, 2, 3}
    got = hash_ranges(gpu, torch.from_numpy(host).cuda(), offs, lens)
    assert not (msg := first_mismatch(got, exp, offs, lens)), msg


@pytest.mark.parametrize("start", [4096, 4099])
def test_last_range_ends_on_the_last_byte_of_the_data(gpu, tables, start):
    """The ragged batch again, the data a view into the middle of a larger tensor: the last range (64 bytes: one whole block) ends on
    the view's last byte."""
    host, offs, lens, exp = tables["ragged"]
    assert int(offs[-1]) + int(lens[-1]) == len(host)
    big = torch.zeros(start + len(host) + 4096, dtype=torch.uint8, device="cuda")
    view = big[start : start + len(host)]
    view.copy_(torch.from_numpy(host))
    got = hash_ranges(gpu, view, offs, lens)
    assert not (msg := first_mismatch(got, exp, offs, lens)), msg


@pytest.mark.parametrize("name", ["edges", "ragged"])
def test_ablation_build_keeps_the_unpipelined_loop(gpu_abl, tables, monkeypatch, name):
    monkeypatch.setenv("LTHIP_B3_PREFETCH", "0")
    gpu_abl.lib.dll.lthip_debug_reload_env()
    host, offs, lens, exp = tables[name]
    got = hash_ranges(gpu_abl, torch.from_numpy(host).cuda(), offs, lens)
    assert not (msg := first_mismatch(got, exp, offs, lens)), f"LTHIP_B3_PREFETCH=0: {msg}"
