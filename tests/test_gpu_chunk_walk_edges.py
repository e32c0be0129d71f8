"""-m gpu: the walking scan (k_buzhash_walk) at the smallest shapes where the walk can go wrong, against the oracle's chunker and BLAKE3,
element for element: offsets, lengths, part_first and hashes.

Plans the rule walks on its own run as they are; the small ones it refuses are walked through the ablation build's LTHIP_K1_WALK=1.
  - parts of 0, 1, min - 1, min, min + 1 and min + 48 bytes, and one of exactly one wave-tile (4 KiB) past min;
  - parts of zero bytes: no candidate, so every chunk ends at max -- the jump behind `end`, and a tail that needs no scan;
  - min < 4 KiB (target 16 KiB): a chunk's first candidate lies in the tile already hashed (the `continue` path); min < 64: the first
    tile starts at the part's first byte and has no halo row;
  - every part at each 16-byte phase of its offset modulo 64 (the DMA's source alignment against the 64-byte runs);
  - 3 parts (most waves draw nothing) and CUs x 16 x 2 + 5 parts of 40 KiB (every wave draws several, the ticket tail is uneven);
  - plans of >= 1 GiB at every slice count the rule can choose, against the single pass, lists equal bit for bit: a walked plan runs
    as one in the product library (and in 2, 3 and 4 slices where the ablation build's LTHIP_SLICES names the count), a plan of few
    long parts runs the tile scan in two.
Random bytes come from k_synth_fill with fixed seeds; the oracle reads the same bytes back from the device."""
import numpy as np
import pytest

from tests.gpu_util import check_part, u32, u64

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
WTILE = 4096
CFG64 = (8192, 32768, 131072)  # chunker_params(65536): the benchmark's
CFGS = [CFG64, (2048, 8192, 32768), (48, 100, 300)]
SLICE_COUNTS = (2, 3, 4)  # named through LTHIP_SLICES (ablation build); 2 GiB holds four slices of >= 512 MiB (plan_slice_points)


def set_env(ctx, mp, **kv):
    for k, v in kv.items():
        mp.setenv(k, str(v))
    ctx.lib.dll.lthip_debug_reload_env()


def unset_env(mp, name, *ctxs):
    """(with LTHIP_LIB_PATH the `gpu` fixture is the ablation build too: it must not see a count named for the reference run)"""
    mp.delenv(name, raising=False)
    for c in ctxs:
        c.lib.dll.lthip_debug_reload_env()


def lists(ctx, plan, data):
    total, off, ln, h, first = ctx.chunk_hash(plan, data)
    first = u32(first)[: plan.nparts + 1]
    assert int(first[-1]) == total and total <= plan.capacity
    return {"offsets": u64(off)[:total], "lengths": u32(ln)[:total], "hashes": u64(h)[:total], "part_first": first}


def phased_layout(sizes, phases):
    """Part i at a 64-byte boundary + 16 x phases[i]."""
    offs, pos = [], 0
    for s, ph in zip(sizes, phases):
        pos = (pos + 63) // 64 * 64 + 16 * ph
        offs.append(pos)
        pos += s
    return offs, (pos + 63) // 64 * 64


def filled(ctx, offs, sizes, zero, total, seed0):
    """A device buffer with k_synth_fill's random bytes (seed0 + i) in the parts that are not `zero`."""
    import torch

    data = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    idx = [i for i in range(len(sizes)) if not zero[i] and sizes[i]]
    if idx:
        ctx.synth_fill(data, [offs[i] for i in idx], [sizes[i] for i in idx], [seed0 + i for i in idx], 0)
    return data


def check_against_oracle(oracle, data, offs, sizes, got, cfg, what):
    host = data.cpu().numpy()
    first = got["part_first"]
    assert int(first[0]) == 0
    for i, (o, s) in enumerate(zip(offs, sizes)):
        a, b = int(first[i]), int(first[i + 1])
        part = (got["offsets"][a:b] - np.uint64(o), got["lengths"][a:b], got["hashes"][a:b])
        check_part(oracle, host[o : o + s], part, *cfg, what=f"{what} part {i} size={s} offset={o}")


@pytest.mark.parametrize("cfg", CFGS)
def test_edge_sizes_at_every_phase(gpu_abl, oracle, monkeypatch, cfg):
    mn, av, mx = cfg
    rnd = [0, 1, mn - 1, mn, mn + 1, mn + 48, mn + WTILE, mn + WTILE + 1, 5 * mn + 77, 2 * mx + mn + 33]
    zer = [mx + 1, 2 * mx + mn, 2 * mx + mn + 100]  # max, then a tail of 1 / of min (no scan) / of min + 100 (one more scan)
    sizes, phases, zero = [], [], []
    for k, s in enumerate(rnd + zer):
        for ph in range(4):
            sizes.append(s)
            phases.append(ph)
            zero.append(k >= len(rnd))
    offs, total = phased_layout(sizes, phases)
    assert {o % 64 for o in offs} == {0, 16, 32, 48}
    data = filled(gpu_abl, offs, sizes, zero, total, 7000 + mn)
    set_env(gpu_abl, monkeypatch, LTHIP_K1_WALK=1)
    plan = gpu_abl.make_plan(offs, sizes, mn, av, mx)
    assert plan.walked_scans == 1
    got = lists(gpu_abl, plan, data)
    plan.close()
    check_against_oracle(oracle, data, offs, sizes, got, cfg, f"cfg={cfg}")
    # the zero parts: every chunk but the tail is max long
    first = got["part_first"]
    for i in range(len(sizes)):
        if zero[i]:
            ln = got["lengths"][int(first[i]) : int(first[i + 1])]
            assert (ln[:-1] == mx).all() and ln.sum() == sizes[i], (sizes[i], ln)


def test_three_parts(gpu_abl, oracle, monkeypatch):
    sizes = [100 * KIB + 5, 0, 300 * KIB + 13]
    offs, total = phased_layout(sizes, [1, 2, 3])
    data = filled(gpu_abl, offs, sizes, [False] * 3, total, 8100)
    set_env(gpu_abl, monkeypatch, LTHIP_K1_WALK=1)
    plan = gpu_abl.make_plan(offs, sizes, *CFG64)
    assert plan.walked_scans == 1
    got = lists(gpu_abl, plan, data)
    plan.close()
    check_against_oracle(oracle, data, offs, sizes, got, CFG64, "three parts")


def test_every_wave_draws_several_parts_uneven_tail(gpu, oracle):
    import torch

    waves = torch.cuda.get_device_properties(0).multi_processor_count * 16
    n = 2 * waves + 5
    sizes = [40 * KIB] * n
    offs, total = phased_layout(sizes, [i & 3 for i in range(n)])
    data = filled(gpu, offs, sizes, [False] * n, total, 9000)
    plan = gpu.make_plan(offs, sizes, *CFG64)  # the product library: the rule decides
    assert plan.slices == 1 and plan.walked_scans == 1, (plan.slices, plan.walked_scans)
    got = lists(gpu, plan, data)
    plan.close()
    check_against_oracle(oracle, data, offs, sizes, got, CFG64, f"{n} parts of 40 KiB")


def test_slice_counts_equal_the_single_pass(gpu, gpu_abl, monkeypatch):
    n = 54000  # > 4 x 2 x 4096 resident waves: every one of four slices is walked
    sizes = [32 * KIB + (i * 7919) % (16 * KIB) for i in range(n)]  # 32 .. 48 KiB: 2.06 GiB, four slices of >= 512 MiB
    for i, s in ((7, 0), (13000, 1), (13500, 8192), (27001, 8193), (40500, 8192 + WTILE), (n - 1, 0)):
        sizes[i] = s
    offs, total = phased_layout(sizes, [i & 3 for i in range(n)])
    assert total >= 2 << 30
    data = filled(gpu_abl, offs, sizes, [False] * n, total, 100000)
    set_env(gpu_abl, monkeypatch, LTHIP_SLICES=1)
    plan = gpu_abl.make_plan(offs, sizes, *CFG64)
    assert plan.slices == 1 and plan.walked_scans == 1
    ref = lists(gpu_abl, plan, data)
    plan.close()
    assert len(ref["lengths"]) > n
    for S in SLICE_COUNTS:
        set_env(gpu_abl, monkeypatch, LTHIP_SLICES=S)
        plan = gpu_abl.make_plan(offs, sizes, *CFG64)
        assert plan.slices == S and plan.walked_scans == S
        got = lists(gpu_abl, plan, data)
        plan.close()
        for k, e in ref.items():
            assert np.array_equal(got[k], e), f"{S} slices: {k} differ from the single pass"
    unset_env(monkeypatch, "LTHIP_SLICES", gpu, gpu_abl)
    plan = gpu.make_plan(offs, sizes, *CFG64)  # the product library's own rule: a walked plan runs as one
    assert plan.slices == 1 and plan.walked_scans == 1, (plan.slices, plan.walked_scans)
    got = lists(gpu, plan, data)
    plan.close()
    for k, e in ref.items():
        assert np.array_equal(got[k], e), f"the product's single pass: {k} differ from the ablation build's"


def test_few_long_parts_run_the_tile_scan_in_two_slices(gpu, gpu_abl, monkeypatch):
    sizes = [300 * MIB + 13, 0, 420 * MIB + 4097, 500 * MIB + 1, 77 * MIB, 12345]  # 1.27 GiB in six parts: never walked
    offs, total = phased_layout(sizes, [0, 1, 2, 3, 1, 2])
    data = filled(gpu_abl, offs, sizes, [False] * len(sizes), total, 200000)
    set_env(gpu_abl, monkeypatch, LTHIP_SLICES=1)
    plan = gpu_abl.make_plan(offs, sizes, *CFG64)
    assert plan.slices == 1 and plan.walked_scans == 0
    ref = lists(gpu_abl, plan, data)
    plan.close()
    unset_env(monkeypatch, "LTHIP_SLICES", gpu, gpu_abl)
    plan = gpu.make_plan(offs, sizes, *CFG64)  # the product library's own rule
    assert plan.slices == 2 and plan.walked_scans == 0, (plan.slices, plan.walked_scans)
    got = lists(gpu, plan, data)
    plan.close()
    assert len(ref["lengths"]) > 10000
    for k, e in ref.items():
        assert np.array_equal(got[k], e), f"two slices of the tile scan: {k} differ from the single pass"
