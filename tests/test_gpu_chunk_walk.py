"""-m gpu: the walking scan (k_buzhash_walk: a wave owns a part and walks it chunk by chunk, skipping the bytes below every chunk's
minimum length) against the tile scan + cut selection of the same plan and against the oracle (ablation build: LTHIP_K1_WALK forces
either scan for any plan).

Thousands of small parts whose sizes sit on every boundary of the walk (the window, min, the 64 bytes in front of min, 4 KiB tiles, max,
tails of at most min bytes) for the parameter sets of test_params_and_kinds -- (48, 48, 48) never scans, (48, 100, 300) jumps to a
tile that starts before its chunk -- on random, zero (no candidate: every chunk is max) and structured data; a plan that the
eligibility rule walks on its own, in one, two and three slices; a re-aim from a walked layout to one the rule rejects and back."""
import numpy as np
import pytest

from tests.gpu_util import check_part, to_device, u32, u64

pytestmark = pytest.mark.gpu

CFGS = [(8192, 32768, 131072), (48, 48, 48), (4096, 16384, 65536), (48, 100, 300), (16384, 65536, 262144), (48, 64, 64), (64, 128, 4096),
        (2048, 2048, 8192), (64, 86, 300)]  # test_gpu_chunk_hash.py::test_params_and_kinds; (64, 86, 300): d = 64, the power-of-two kernels
KIB, MIB = 1 << 10, 1 << 20


def set_env(ctx, mp, **kv):
    for k, v in kv.items():
        mp.setenv(k, str(v))
    ctx.lib.dll.lthip_debug_reload_env()


def lists(ctx, plan, data):
    total, off, ln, h, first = ctx.chunk_hash(plan, data)
    return {"offsets": u64(off)[:total], "lengths": u32(ln)[:total], "hashes": u64(h)[:total], "part_first": u32(first)[: plan.nparts + 1]}


def assert_same(got, exp, what):
    for k, e in exp.items():
        g = got[k]
        assert len(g) == len(e), f"{what}: {k}: {len(g)} entries, want {len(e)}"
        bad = np.nonzero(g != e)[0]
        assert len(bad) == 0, f"{what}: {k} differ at {bad[:5]}"


def boundary_sizes(mn, mx):
    s = {0, 1, 47, 48, mn, mn + 1, mn + 47, mn + 48, mn + 64, mx - 1, mx, mx + 1, 2 * mx + 17}
    for k in (1, 2, 3, 5, 8, 16, 33):
        s |= {4096 * k - 1, 4096 * k, 4096 * k + 1}
    for t in (1, mn - 1, mn, mn + 1):  # behind chunks of max bytes (zero data) a tail around min
        s |= {mx + t, 2 * mx + t}
    return sorted(x for x in s if x <= 2 * mx + mn + 1 or x <= 8 * 4096 + 1)


@pytest.mark.parametrize("cfg", CFGS)
def test_boundary_sizes_both_scans_and_oracle(gpu_abl, oracle, monkeypatch, cfg):
    mn, av, mx = cfg
    sizes = boundary_sizes(mn, mx)
    big = max(sizes)
    bases = [oracle.synth(big + 4096, 100 * mn + kind, kind) for kind in (0, 1, 2)]
    parts = []
    for i, s in enumerate(sizes):
        for rep in range(9):  # random bytes from nine places, so that cuts fall at different distances from the boundaries
            o = (rep * 911 + i * 37) % 4096
            parts.append(bases[0][o : o + s].copy())
        parts.append(bases[1][i : i + s].copy())
        parts.append(bases[2][i : i + s].copy())
        parts.append(np.zeros(s, np.uint8))
    dev, offs = to_device(parts)
    got = {}
    for walk in (0, 1):
        set_env(gpu_abl, monkeypatch, LTHIP_K1_WALK=walk)
        plan = gpu_abl.make_plan(offs, [len(p) for p in parts], mn, av, mx)
        assert plan.walked_scans == walk
        got[walk] = lists(gpu_abl, plan, dev)
        plan.close()
    assert_same(got[1], got[0], f"cfg={cfg}: walking scan against tile scan")
    g, first = got[1], got[1]["part_first"]
    for i, p in enumerate(parts):
        a, b = int(first[i]), int(first[i + 1])
        part = (g["offsets"][a:b] - np.uint64(offs[i]), g["lengths"][a:b], g["hashes"][a:b])
        check_part(oracle, p, part, mn, av, mx, what=f"cfg={cfg} part {i} size={len(p)}")


# ---- plans the rule decides on ----
CFG = (8192, 32768, 131072)
N_SMALL = 54000  # > 3 x 4 x 4096 resident waves (256 CUs x 16): every one of three slices is walked
SIZES_SMALL = [24 * KIB + (i * 7919) % (20 * KIB) for i in range(N_SMALL)]  # 24 .. 44 KiB: 1.8 GiB, 3 slices of >= 0.5 GiB
for _i, _s in ((5, 0), (4711, 1), (4712, 47), (20000, 8192), (20001, 8193), (33333, 61441), (53999, 0)):
    SIZES_SMALL[_i] = _s
SIZES_BIG = [300 * MIB + 13, 0, 420 * MIB + 4097, 500 * MIB + 1, 77 * MIB, 12345]  # six parts: rejected by the rule


def layout(sizes):
    ends = np.cumsum([(s + 15) // 16 * 16 for s in sizes])
    return [0] + [int(e) for e in ends[:-1]], int(ends[-1])


@pytest.fixture(scope="module")
def tree(gpu_abl):
    """A buffer of structured bytes and the tile scan's lists (one slice) of both layouts over it."""
    import torch

    total = max(layout(SIZES_SMALL)[1], layout(SIZES_BIG)[1])
    data = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    n = 64
    gpu_abl.synth_fill(data, [i * (total // n // 16 * 16) for i in range(n)], [total // n // 16 * 16] * n, [900 + i for i in range(n)], 1)
    ref = {}
    with pytest.MonkeyPatch.context() as mp:
        set_env(gpu_abl, mp, LTHIP_K1_WALK=0, LTHIP_SLICES=1)
        for name, sizes in (("small", SIZES_SMALL), ("big", SIZES_BIG)):
            plan = gpu_abl.make_plan(layout(sizes)[0], sizes, *CFG)
            assert plan.slices == 1 and plan.walked_scans == 0
            ref[name] = lists(gpu_abl, plan, data)
            plan.close()
    gpu_abl.lib.dll.lthip_debug_reload_env()
    assert len(ref["small"]["lengths"]) > N_SMALL and len(ref["big"]["lengths"]) > 10000
    return data, ref


def launches(ctx, fn):
    ctx.timing(True)
    ctx.timing_reset()
    out = fn()
    t = ctx.timing_get()
    ctx.timing(False)
    return out, {k: int(t[k][1]) for k in ("buzhash", "select")}


@pytest.mark.parametrize("S", [1, 2, 3])
def test_rule_walks_many_small_parts_in_slices(gpu_abl, tree, monkeypatch, S):
    data, ref = tree
    set_env(gpu_abl, monkeypatch, LTHIP_SLICES=S)
    plan = gpu_abl.make_plan(layout(SIZES_SMALL)[0], SIZES_SMALL, *CFG)
    assert plan.slices == S and plan.walked_scans == S
    got, n = launches(gpu_abl, lambda: lists(gpu_abl, plan, data))
    assert n == {"buzhash": S, "select": 0}, n  # the walking scan selects the cuts itself
    assert_same(got, ref["small"], f"walked, S={S}")
    plan.close()


def test_reaim_walked_to_rejected_and_back(gpu_abl, tree, monkeypatch):
    data, ref = tree
    set_env(gpu_abl, monkeypatch, LTHIP_SLICES=2)
    plan = gpu_abl.make_plan(layout(SIZES_SMALL)[0], SIZES_SMALL, *CFG)
    assert plan.walked_scans == 2
    assert_same(lists(gpu_abl, plan, data), ref["small"], "walked")
    plan.reaim(layout(SIZES_BIG)[0], SIZES_BIG)  # six parts: the tile scan, whatever it is sliced into
    assert plan.walked_scans == 0
    got, n = launches(gpu_abl, lambda: lists(gpu_abl, plan, data))
    assert n["select"] == n["buzhash"] == plan.slices, n
    assert_same(got, ref["big"], "re-aimed at a layout the rule rejects")
    plan.reaim(layout(SIZES_SMALL)[0], SIZES_SMALL)
    assert plan.slices == 2 and plan.walked_scans == 2
    assert_same(lists(gpu_abl, plan, data), ref["small"], "re-aimed at the walked layout again")
    plan.close()


def test_rejected_plan_runs_the_tile_scan_and_can_be_forced(gpu_abl, tree, monkeypatch):
    data, ref = tree
    plan = gpu_abl.make_plan(layout(SIZES_BIG)[0], SIZES_BIG, *CFG)
    assert plan.walked_scans == 0
    got, n = launches(gpu_abl, lambda: lists(gpu_abl, plan, data))
    assert n["select"] == n["buzhash"] == plan.slices, n
    assert_same(got, ref["big"], "rejected plan")
    set_env(gpu_abl, monkeypatch, LTHIP_K1_WALK=1)  # six waves walk 1.3 GiB: slow, and the same lists
    assert plan.walked_scans == plan.slices
    assert_same(lists(gpu_abl, plan, data), ref["big"], "rejected plan, walking scan forced")
    plan.close()
