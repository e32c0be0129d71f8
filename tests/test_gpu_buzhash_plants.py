"""-m gpu: the Buzhash scans on the planted parts of tests/buzhash_plants.py -- bytes built so that the cuts fall where the cases choose
(tests/test_buzhash_plants_cases.py proves on the CPU what every case reaches): every (lane, step) class of a wave-tile and every
alignment of the walking scan's tile, the edges of the cut test's arithmetic, the arrangements of k_select_cuts' search, many cuts in
one tile, cuts that make the walk's prefetch wrong; every case for a discriminator that is a power of two (the MODE == 1 kernels) and
for one that is not.

Every case goes, part by part and element for element (offsets, lengths, hashes, part_first: check_part against the oracle's chunks,
computed once per case), through
  - the tile scan + k_select_cuts of the ablation build (LTHIP_K1_WALK=0),
  - the walking scan in its four instantiations (LTHIP_K1_WALK=1; LTHIP_WALK_HASH = 0 / 1; LTHIP_K1_WALK_GUESS unset / 0),
  - the product library under its own rule;
lthip_chunk_from_buffer is held to the oracle's NextChunkFromBuffer for the power-of-two parameter sets."""
import numpy as np
import pytest
import torch

from tests import buzhash_plants as P
from tests.gpu_util import check_part
from tests.test_gpu_chunk_walk import launches, lists, set_env

pytestmark = pytest.mark.gpu

# name -> (the switches of the ablation build, or None = the product library; whether the scan walks)
SCANS = {
    "tile": ({"LTHIP_K1_WALK": 0}, False),
    "walk": ({"LTHIP_K1_WALK": 1, "LTHIP_WALK_HASH": 0}, True),
    "walk-guess0": ({"LTHIP_K1_WALK": 1, "LTHIP_WALK_HASH": 0, "LTHIP_K1_WALK_GUESS": 0}, True),
    "hash_walk": ({"LTHIP_K1_WALK": 1, "LTHIP_WALK_HASH": 1}, True),
    "hash_walk-guess0": ({"LTHIP_K1_WALK": 1, "LTHIP_WALK_HASH": 1, "LTHIP_K1_WALK_GUESS": 0}, True),
    "product": (None, None),
}


@pytest.fixture(scope="module")
def staged():
    """A case's groups on the device, each in one buffer whose part offsets cycle through the four 16-byte phases modulo 64, and the
    oracle's chunks of its parts: made once, shared by the six scans, left unchanged."""
    made = {}

    def get(name):
        if name not in made:
            groups = []
            for g in P.CASES[name]().groups:
                offs, total = P.place(g.parts)
                host = np.zeros(total + 64, np.uint8)
                for o, p in zip(offs, g.parts):
                    host[o : o + len(p)] = p
                assert total + 64 <= 64 << 20
                groups.append((g, offs, torch.from_numpy(host).cuda()))
            made[name] = (groups, P.Recorded(name))
        return made[name]

    return get


@pytest.mark.parametrize("scan", list(SCANS))
@pytest.mark.parametrize("name", list(P.CASES))
def test_planted_case(request, staged, monkeypatch, name, scan):
    env, walks = SCANS[scan]
    ctx = request.getfixturevalue("gpu" if env is None else "gpu_abl")
    if env is not None:
        monkeypatch.delenv("LTHIP_K1_WALK_GUESS", raising=False)
        set_env(ctx, monkeypatch, **env)
    groups, recorded = staged(name)
    for g, offs, dev in groups:
        plan = ctx.make_plan(offs, [len(p) for p in g.parts], *g.cfg)
        if walks is not None:
            assert plan.walked_scans == (plan.slices if walks else 0)
        got, n = launches(ctx, lambda: lists(ctx, plan, dev))
        assert n == {"buzhash": plan.slices, "select": plan.slices - plan.walked_scans}, (scan, n)  # a walking scan selects the cuts itself
        plan.close()
        first = got["part_first"]
        assert len(first) == len(g.parts) + 1 and int(first[-1]) == len(got["lengths"])
        for i, p in enumerate(g.parts):
            a, b = int(first[i]), int(first[i + 1])
            part = (got["offsets"][a:b] - np.uint64(offs[i]), got["lengths"][a:b], got["hashes"][a:b])
            check_part(recorded, p, part, *g.cfg, what=f"{name} {scan} cfg={g.cfg} part {i} {g.labels[i]!r:.80}")


@pytest.mark.parametrize("cfg", P.FROM_BUFFER_CFGS)
def test_from_buffer_power_of_two(gpu, oracle, cfg):
    """k_chunk_from_buffer's pow2 branch: call by call over random bytes, and on zero buffers with one window planted behind the 47
    lengths whose window still holds the buffer's first bytes."""
    mn, av, mx = cfg
    assert P.is_pow2(P.disc(av))
    data = np.random.default_rng(mn + av).integers(0, 256, size=min(40 * av, 1 << 20) + 77, dtype=np.uint8)
    dev = torch.from_numpy(np.concatenate([data, np.zeros(64, np.uint8)])).cuda()
    pos, calls, cut = 0, 0, 0
    while pos < len(data) and calls < 48:
        want = int(oracle.dll.lto_hpcdc_next_from_buffer(data[pos:].ctypes.data, len(data) - pos, mn, av, mx))
        assert gpu.chunk_from_buffer(dev[pos:], len(data) - pos, mn, av, mx) == want, (cfg, pos)
        cut += mn < want < min(mx, len(data) - pos)
        pos += want
        calls += 1
    assert cut >= 10  # (chunks that a candidate ended, not min, max or the buffer's end)
    for c, a, p in P.from_buffer_plants():
        if c == cfg:
            d = torch.from_numpy(np.concatenate([a, np.zeros(64, np.uint8)])).cuda()
            assert gpu.chunk_from_buffer(d, len(a), mn, av, mx) == p, (cfg, p)
