"""-m gpu: the walking scan that hashes the chunks it cuts (k_buzhash_hash_walk: the wave that emits a chunk puts it on a pending
list and hashes 64 pending leaves at a time, a leaf per lane; the chaining values go to per-part runs that a kernel behind compaction
moves into the dense leaf order) against the walking scan followed by the leaf pass of its own, and against the oracle (ablation build:
LTHIP_WALK_HASH = 0 / 1 forces either form, LTHIP_K1_WALK = 1 the walking scan for any plan, LTHIP_K1_WALK_GUESS = 0 the other
prefetch form: the two kernels are one walk body, and both forms of both meet the oracle here).

Offsets, lengths, hashes and part_first must be bit-identical for the parameter sets of test_gpu_chunk_walk.py -- (48, 48, 48) and
(48, 64, 64) have leaves of 48-64 bytes -- on part sizes at every edge of the leaf (0, 1, 47, 48, min, min + 1, 1023 .. 1025, 4095 ..
4097, max, max + 1, multiples of 1024), on random bytes and on zeros (no candidate: every chunk is max bytes, so chunks of 128 and 256
leaves span rounds), in thousands of parts, so that every wave draws several and its list carries from part to part.  A part's offset
is a multiple of 16 (the plan's rule); the chunks inside start at every residue mod 16, which the test asserts."""
import numpy as np
import pytest

from tests.gpu_util import check_part, to_device, u32, u64
from tests.test_gpu_chunk_walk import CFGS, assert_same, layout, lists, set_env

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20


def both_forms(ctx, mp, offs, sizes, cfg, data, **env):
    """The lists of the separate (0) and the fused (1) form of a plan whose scan walks."""
    got = {}
    for fused in (0, 1):
        set_env(ctx, mp, LTHIP_WALK_HASH=fused, **env)
        plan = ctx.make_plan(offs, sizes, *cfg)
        assert plan.walked_scans == plan.slices
        got[fused] = lists(ctx, plan, data)
        plan.close()
    return got


def edge_sizes(mn, mx):
    s = {0, 1, 47, 48, mn, mn + 1, 1023, 1024, 1025, 4095, 4096, 4097, mx - 1, mx, mx + 1, 2 * mx + 17, 3 * 1024, 64 * 1024, 65 * 1024}
    return sorted(s)


def prefetch_env(mp, guess):
    """The walk's prefetch form: None = the product's (LTHIP_K1_WALK_GUESS unset), 0 = the other one.  With the fused and the separate
    form of both_forms all four GUESS x HASH instantiations of the one walk body run."""
    if guess is None:
        mp.delenv("LTHIP_K1_WALK_GUESS", raising=False)
        return {}
    return {"LTHIP_K1_WALK_GUESS": guess}


# every cfg on the product's prefetch form; several cuts per tile and the headline's parameters on the other form as well
CFGS_GUESS = [pytest.param(c, None, id=f"cfg{i}") for i, c in enumerate(CFGS)]
CFGS_GUESS += [pytest.param(c, 0, id=f"cfg{CFGS.index(c)}-guess0") for c in ((64, 128, 4096), (8192, 32768, 131072))]


@pytest.mark.parametrize("cfg,guess", CFGS_GUESS)
def test_fused_against_separate_and_oracle(gpu_abl, oracle, monkeypatch, cfg, guess):
    mn, av, mx = cfg
    sizes = edge_sizes(mn, mx)
    big = max(sizes)
    rnd = np.random.default_rng(mn * 7 + mx).integers(0, 256, size=big + 8192, dtype=np.uint8)
    parts = []
    for i, s in enumerate(sizes):
        for rep in range(4):  # random bytes from four places: cuts at different distances from the edges
            o = (rep * 911 + i * 37) % 4096
            parts.append(rnd[o : o + s].copy())
        parts.append(np.zeros(s, np.uint8))
        parts.append(np.zeros(2 * mx + s, np.uint8))  # behind two chunks of max bytes
    n_edge = len(parts)
    # thousands of small parts around them: more parts than the device holds waves, so lists carry across draws in every wave
    small = [x for x in sizes if x <= 4097] + [777, 2000, 3333]
    for i in range(9000):
        s = small[i % len(small)] if i % 3 else 1 + (i * 2654435761) % 6000
        o = (i * 131) % 2048
        parts.append(rnd[o : o + s].copy() if i % 11 else np.zeros(s, np.uint8))
    dev, offs = to_device(parts)
    got = both_forms(gpu_abl, monkeypatch, offs, [len(p) for p in parts], cfg, dev, LTHIP_K1_WALK=1, **prefetch_env(monkeypatch, guess))
    assert_same(got[1], got[0], f"cfg={cfg} guess={guess}: fused against separate")
    g, first = got[1], got[1]["part_first"]
    if mx > mn:  # (random data, chunks of varying length: they start everywhere)
        assert set((g["offsets"] % np.uint64(16)).tolist()) == set(range(16))
    for i in list(range(n_edge)) + list(range(n_edge, len(parts), 97)):
        a, b = int(first[i]), int(first[i + 1])
        part = (g["offsets"][a:b] - np.uint64(offs[i]), g["lengths"][a:b], g["hashes"][a:b])
        check_part(oracle, parts[i], part, mn, av, mx, what=f"cfg={cfg} part {i} size={len(parts[i])}")


@pytest.mark.parametrize(
    "zeros,tail,guess",
    [pytest.param(z, t, g, id=f"{z}-{t}" + ("" if g is None else f"-guess{g}"))
     for g in (None, 0) for z in (True, False) for t in (1, 63 * KIB, 64 * KIB, 64 * KIB + 1)],
)
def test_one_wave_last_round(gpu_abl, oracle, monkeypatch, tail, zeros, guess):
    """ONE part, so one wave: on zeros a chunk of max = 128 leaves (two full rounds), then a tail of 1, 63, 64 or 65 leaves."""
    cfg = (8192, 32768, 131072)
    size = cfg[2] + tail
    part = np.zeros(size, np.uint8) if zeros else np.random.default_rng(tail).integers(0, 256, size=size, dtype=np.uint8)
    dev, offs = to_device([part])
    got = both_forms(gpu_abl, monkeypatch, offs, [size], cfg, dev, LTHIP_K1_WALK=1, **prefetch_env(monkeypatch, guess))
    assert_same(got[1], got[0], f"tail={tail} zeros={zeros} guess={guess}")
    if zeros:
        assert got[1]["lengths"].tolist() == [cfg[2], tail]
    check_part(oracle, part, (got[1]["offsets"], got[1]["lengths"], got[1]["hashes"]), *cfg, what=f"tail={tail} zeros={zeros}")


# ---- many parts on structured bytes that live on the device ----
CFG_LONG = (96 * KIB, 128 * KIB, 256 * KIB)  # every chunk but a part's last is above 96 leaves
N_PAIRS = 4600  # > 2 x 4096 resident waves (256 CUs x 16) in parts: every wave draws several
SIZES_CARRY = [s for i in range(N_PAIRS) for s in (20 * KIB + (i * 7919) % (40 * KIB) + i % 3, 300 * KIB + (i * 104729) % (8 * KIB))]
# (a part of 20 .. 60 KiB is one chunk below min: fewer than 64 leaves pending; the next part's first chunk has more than 96)
CFG = (8192, 32768, 131072)
SIZES_WALK = [24 * KIB + (i * 7919) % (10 * KIB) for i in range(10000)]  # 24 .. 34 KiB, 285 MiB: the rule walks it (one slice)
for _i, _s in ((5, 0), (4711, 1), (4712, 47), (7000, 8192), (7001, 8193), (9999, 0)):
    SIZES_WALK[_i] = _s
SIZES_BIG = [30 * MIB + 13, 0, 42 * MIB + 4097, 50 * MIB + 1, 7 * MIB, 12345]  # six parts: rejected by the rule


@pytest.fixture(scope="module")
def tree(gpu_abl):
    import torch

    total = max(layout(s)[1] for s in (SIZES_CARRY, SIZES_WALK, SIZES_BIG))
    data = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    n = 64
    gpu_abl.synth_fill(data, [i * (total // n // 16 * 16) for i in range(n)], [total // n // 16 * 16] * n, [700 + i for i in range(n)], 1)
    return data


@pytest.mark.parametrize("slices", [0, 2])
def test_list_carries_from_part_to_part(gpu_abl, tree, monkeypatch, slices):
    offs = layout(SIZES_CARRY)[0]
    env = {"LTHIP_SLICES": slices} if slices else {}
    if not slices:
        monkeypatch.delenv("LTHIP_SLICES", raising=False)
    got = both_forms(gpu_abl, monkeypatch, offs, SIZES_CARRY, CFG_LONG, tree, LTHIP_K1_WALK=1, **env)
    assert_same(got[1], got[0], f"carry, LTHIP_SLICES={slices}")
    first, ln = got[1]["part_first"], got[1]["lengths"]
    assert all(first[i + 1] - first[i] == 1 for i in range(0, 64, 2)) and (ln[first[1:-1:2]] > 96 * KIB).all()


def test_reaim_walked_rejected_walked(gpu_abl, tree, monkeypatch):
    ref = {}
    set_env(gpu_abl, monkeypatch, LTHIP_WALK_HASH=0)
    for name, sizes in (("walk", SIZES_WALK), ("big", SIZES_BIG)):
        plan = gpu_abl.make_plan(layout(sizes)[0], sizes, *CFG)
        ref[name] = lists(gpu_abl, plan, tree)
        plan.close()
    set_env(gpu_abl, monkeypatch, LTHIP_WALK_HASH=1)
    plan = gpu_abl.make_plan(layout(SIZES_WALK)[0], SIZES_WALK, *CFG)
    assert plan.walked_scans == 1
    assert_same(lists(gpu_abl, plan, tree), ref["walk"], "walked")
    plan.reaim(layout(SIZES_BIG)[0], SIZES_BIG)
    assert plan.walked_scans == 0
    assert_same(lists(gpu_abl, plan, tree), ref["big"], "re-aimed at a layout the rule rejects")
    plan.reaim(layout(SIZES_WALK)[0], SIZES_WALK)
    assert plan.walked_scans == 1
    assert_same(lists(gpu_abl, plan, tree), ref["walk"], "re-aimed at the walked layout again")
    plan.close()


def test_product_walks_without_hashes(gpu, tree):
    """The product library runs k_buzhash_walk only for a walked plan whose hashes nobody asks for: the cuts of the scan that hashes."""
    plan = gpu.make_plan(layout(SIZES_WALK)[0], SIZES_WALK, *CFG)
    assert plan.walked_scans == 1
    hashed = lists(gpu, plan, tree)
    total, off, ln, h, first = gpu.chunk_hash(plan, tree, want_hashes=False)
    assert plan.walked_scans == 1 and h is None
    plain = {"offsets": u64(off)[:total], "lengths": u32(ln)[:total], "part_first": u32(first)[: plan.nparts + 1]}
    assert_same(plain, {k: hashed[k] for k in plain}, "the walk without hashes against the walk that hashes")
    plan.close()
