"""-m gpu: the Buzhash scans on the parts of tests/buzhash_rot_table.py -- random bytes that reach every entry of the LDS table of rotations
(R[r][v] = rotr(T[v], r)), bytes of one LDS bank, one byte broadcast around random ones (tests/test_buzhash_rot_table_cases.py proves
on the CPU what the parts reach and that one wrong entry changes part A's chunk list).

Every part lies at the four 16-byte phases of the part offset; for two small parameter sets (a discriminator that is a power of two
and one that is not) and the headline's, the buffer goes through the six scans of tests/test_gpu_buzhash_plants.py -- the tile scan, the
four walking scans, the product library under its own rule -- and every part is held to the oracle's chunks (computed once per
parameter set): offsets, lengths, hashes, part_first."""
import numpy as np
import pytest
import torch

from tests import buzhash_plants as P
from tests import buzhash_rot_table as R
from tests.gpu_util import check_part
from tests.test_gpu_buzhash_plants import SCANS
from tests.test_gpu_chunk_walk import launches, lists, set_env

pytestmark = pytest.mark.gpu

CFGS = R.CFGS + [R.HEADLINE]


class Once:
    """What check_part asks of an oracle, each (part, parameter set) computed once for the six scans."""

    def __init__(self, oracle):
        self.oracle, self.made = oracle, {}

    def chunk_and_hash(self, data, mn, av, mx):
        key = (id(data), mn, av, mx)
        if key not in self.made:
            self.made[key] = self.oracle.chunk_and_hash(data, mn, av, mx)
        return self.made[key]


@pytest.fixture(scope="module")
def staged(oracle):
    """Every part four times, at the four 16-byte phases modulo 64, in one device buffer: made once, left unchanged."""
    parts, labels = [], []
    for name, a in R.parts().items():
        parts += [a] * 4
        labels += [f"{name}@{16 * ph}" for ph in range(4)]
    offs, total = P.place(parts)
    assert [o % 64 for o in offs] == [0, 16, 32, 48] * len(R.parts()) and total < 2 << 20
    host = np.zeros(total + 64, np.uint8)
    for o, p in zip(offs, parts):
        host[o : o + len(p)] = p
    return parts, labels, offs, torch.from_numpy(host).cuda(), Once(oracle)


@pytest.mark.parametrize("scan", list(SCANS))
@pytest.mark.parametrize("cfg", CFGS)
def test_rot_table_parts(request, staged, monkeypatch, cfg, scan):
    env, walks = SCANS[scan]
    ctx = request.getfixturevalue("gpu" if env is None else "gpu_abl")
    if env is not None:
        monkeypatch.delenv("LTHIP_K1_WALK_GUESS", raising=False)
        set_env(ctx, monkeypatch, **env)
    parts, labels, offs, dev, once = staged
    plan = ctx.make_plan(offs, [len(p) for p in parts], *cfg)
    if walks is not None:
        assert plan.walked_scans == (plan.slices if walks else 0)
    got, n = launches(ctx, lambda: lists(ctx, plan, dev))
    assert n == {"buzhash": plan.slices, "select": plan.slices - plan.walked_scans}, (scan, n)
    plan.close()
    first = got["part_first"]
    assert len(first) == len(parts) + 1 and int(first[-1]) == len(got["lengths"])
    for i, p in enumerate(parts):
        a, b = int(first[i]), int(first[i + 1])
        part = (got["offsets"][a:b] - np.uint64(offs[i]), got["lengths"][a:b], got["hashes"][a:b])
        check_part(once, p, part, *cfg, what=f"{scan} cfg={cfg} part {labels[i]}")
