"""-m gpu: lthip_chunk_hash in S slices on two streams against the single pass of the same plan (ablation build: LTHIP_SLICES).

A plan of >= 1 GiB in >= 2 parts runs as S slices (lthip_ctx.hip, chunk_hash_sliced); its lists must be those of the single pass byte
for byte: for S = 2, 3 and 8, across uneven parts and zero-size parts, after a re-aim that no longer fits the slices (the plan runs as
one) and back again, and with device allocations made to fail one after another inside a sliced call on a cold context (the pass falls
back to the single pass or the call fails with ENOMEM; the next call is right again)."""
import ctypes as C
import errno

import numpy as np
import pytest

from tests.gpu_util import u32, u64

pytestmark = pytest.mark.gpu

MIB = 1 << 20
# 4.2 GiB in 12 parts, two of them empty: total / 8 >= LTHIP_SLICE_MIN_BYTES / 2, so LTHIP_SLICES = 8 gives 8 slices
SIZES_A = [1100 * MIB + 13, 0, 37 * MIB + 5, 610 * MIB + 4097, 5 * MIB + 1, 0, 880 * MIB + 999, 333 * MIB + 77, MIB, 720 * MIB + 3,
           12345, 640 * MIB + 16383]
# the same parts in reverse: the parent plan's tables fit them, the slices of SIZES_A do not (other parts / tiles per slice)
SIZES_B = SIZES_A[::-1]
CFG = (8192, 32768, 131072)  # chunker_params(65536)


def layout(sizes):
    """-> (16-byte aligned offsets of the parts back to back, bytes in all)"""
    ends = np.cumsum([(s + 15) // 16 * 16 for s in sizes])
    return [0] + [int(e) for e in ends[:-1]], int(ends[-1])


def make_plan(ctx, monkeypatch, slices, sizes):
    monkeypatch.setenv("LTHIP_SLICES", str(slices))
    ctx.lib.dll.lthip_debug_reload_env()
    return ctx.make_plan(layout(sizes)[0], sizes, *CFG)


def lists(ctx, plan, data):
    total, off, ln, h, first = ctx.chunk_hash(plan, data)
    return {"offsets": u64(off)[:total], "lengths": u32(ln)[:total], "hashes": u64(h)[:total], "part_first": u32(first)[: plan.nparts + 1]}


def assert_same(got, exp, what):
    for k, e in exp.items():
        g = got[k]
        assert len(g) == len(e), f"{what}: {k}: {len(g)} entries, want {len(e)}"
        bad = np.nonzero(g != e)[0]
        assert len(bad) == 0, f"{what}: {k} differ at {bad[:5]}"


@pytest.fixture(scope="module")
def tree(gpu_abl):
    """The device buffer (SIZES_A's parts synthesised from seeds, zeros between) and the single pass's lists of both layouts."""
    import torch

    offs, total = layout(SIZES_A)
    data = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    gpu_abl.synth_fill(data, offs, SIZES_A, [7000 + i for i in range(len(SIZES_A))], 1)
    ref = {}
    with pytest.MonkeyPatch.context() as mp:
        for name, sizes in (("A", SIZES_A), ("B", SIZES_B)):
            plan = make_plan(gpu_abl, mp, 1, sizes)
            assert plan.slices == 1
            ref[name] = lists(gpu_abl, plan, data)
            plan.close()
    gpu_abl.lib.dll.lthip_debug_reload_env()
    assert len(ref["A"]["lengths"]) > 10000 and ref["A"]["part_first"][1] == ref["A"]["part_first"][2]  # (part 1 is empty)
    return data, ref


@pytest.mark.parametrize("S", [2, 3, 8])
def test_slices_equal_the_single_pass(gpu_abl, tree, monkeypatch, S):
    data, ref = tree
    plan = make_plan(gpu_abl, monkeypatch, S, SIZES_A)
    assert plan.slices == S
    assert_same(lists(gpu_abl, plan, data), ref["A"], f"S={S}")
    plan.reaim(layout(SIZES_B)[0], SIZES_B)  # does not fit the slices: runs as one
    assert plan.slices == 1
    assert_same(lists(gpu_abl, plan, data), ref["B"], f"S={S}, re-aimed unsliced")
    plan.reaim(layout(SIZES_A)[0], SIZES_A)  # fits them again
    assert plan.slices == S
    assert_same(lists(gpu_abl, plan, data), ref["A"], f"S={S}, re-aimed sliced again")
    plan.close()


def test_sliced_call_allocation_failures(gpu_abl, tree, monkeypatch):
    """Allocation k + 1 of a cold run (plan creation + one sliced call on a fresh context, whose slice context and scratch do not exist
    yet) fails, for every k: plan creation gives ENOMEM or a plan of 1 or S slices, the sliced call gives the single pass's lists or
    ENOMEM with a message; the next call without injection gives the right lists."""
    from longtail_amd.lib import Context, LongtailHipError

    data, ref = tree
    d = gpu_abl.lib.dll
    assert d.lthip_debug_fail_alloc(-1, 0) == 0, "the ablation build must have the injection switch"
    S = 3

    def calls():
        failed = C.c_int64(0)
        n = d.lthip_debug_alloc_calls(C.byref(failed))
        return int(n), int(failed.value)

    ctx = Context(0, lib=gpu_abl.lib)
    n0 = calls()[0]
    plan = make_plan(ctx, monkeypatch, S, SIZES_A)
    assert plan.slices == S
    assert_same(lists(ctx, plan, data), ref["A"], "cold run")
    n_cold = calls()[0] - n0
    plan.close(), ctx.close()
    assert n_cold > 2 * (S + 1), n_cold  # (two tables per plan, then the call's scratch)

    outcomes = {"plan_enomem": 0, "call_enomem": 0, "fallback": 0}
    for k in range(n_cold):
        ctx, plan = Context(0, lib=gpu_abl.lib), None
        d.lthip_debug_fail_alloc(k, 1)
        try:
            try:
                plan = make_plan(ctx, monkeypatch, S, SIZES_A)
            except LongtailHipError as e:
                assert e.code == errno.ENOMEM, f"allocation {k + 1} of {n_cold}: plan creation gave {e}"
                outcomes["plan_enomem"] += 1
            if plan is not None:
                assert plan.slices in (1, S), f"allocation {k + 1} of {n_cold}: {plan.slices} slices"
                failed0 = calls()[1]
                try:
                    got = lists(ctx, plan, data)
                except LongtailHipError as e:
                    assert e.code == errno.ENOMEM, f"allocation {k + 1} of {n_cold}: chunk_hash gave {e}"
                    assert d.lthip_ctx_error(ctx.h), f"allocation {k + 1} of {n_cold}: ENOMEM without a message"
                    outcomes["call_enomem"] += 1
                else:
                    assert_same(got, ref["A"], f"allocation {k + 1} of {n_cold} failing")
                    outcomes["fallback"] += plan.slices == S and calls()[1] > failed0
        finally:
            d.lthip_debug_fail_alloc(-1, 0)
        if plan is None:
            plan = make_plan(ctx, monkeypatch, S, SIZES_A)
        assert_same(lists(ctx, plan, data), ref["A"], f"the call after allocation {k + 1} of {n_cold} failed")
        plan.close(), ctx.close()
    # every kind was reached: a failed plan, a sliced call that fell back to the single pass, a call that failed
    assert all(outcomes.values()), outcomes
