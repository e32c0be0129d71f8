"""-m gpu: the one realigning byte copy of the device side (lthip_wg_copy, longtail_amd/csrc/k_copy.h) through its plainest door,
lthip_gather_ranges: every source residue mod 16 x every destination residue mod 16 x lengths at which the head, each realignment of the
source, the 16-byte body and the tail each run and each do not run.  The copied bytes must be the source's and no byte around a range
may be touched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 3, 15, 16, 17, 31, 33, 255, 4097]
GUARD = 0xC3


@pytest.mark.timeout(120)
def test_gather_ranges_every_alignment_and_no_byte_beside_a_range(gpu):
    rng = np.random.default_rng(16)
    cases = [(s, d, n) for s in range(16) for d in range(16) for n in LENGTHS]
    assert len(cases) == 2560
    # every range has a slot of its own in the source and in the destination: its length + 32 rounded up to 16, so that the slot starts
    # on a 16-byte boundary and the range, `residue` bytes into the slot's second 16, has at least 16 bytes of the slot on either side
    lens = np.array([n for _, _, n in cases], np.uint32)
    slots = np.concatenate([[0], np.cumsum((lens.astype(np.int64) + 32 + 15) // 16 * 16 + 16)])
    src_off = (slots[:-1] + 16 + np.array([s for s, _, _ in cases])).astype(np.uint64)
    dst_off = (slots[:-1] + 16 + np.array([d for _, d, _ in cases])).astype(np.uint64)
    src = rng.integers(0, 256, int(slots[-1]), dtype=np.uint8)
    want = np.full(int(slots[-1]), GUARD, np.uint8)
    for so, do, n in zip(src_off.tolist(), dst_off.tolist(), lens.tolist()):
        want[do : do + n] = src[so : so + n]
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((int(slots[-1]),), GUARD, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    gpu.gather_ranges(d_src, torch.from_numpy(src_off.view(np.int64)).cuda(), torch.from_numpy(lens.view(np.int32)).cuda(), d_dst,
                      torch.from_numpy(dst_off.view(np.int64)).cuda())
    gpu.sync()
    got = d_dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    first = cases[int(np.searchsorted(slots, bad[0], side="right")) - 1] if bad.size else None
    assert bad.size == 0, f"{bad.size} bytes differ, the first in the slot of (source residue, destination residue, length) = {first}"
