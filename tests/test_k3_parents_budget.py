"""The resources of the small-tree parents kernel, read from the compiler's resource summary of k_blake3.hip (no GPU).

k_blake3_parents_window is bound by the latency of its own chain, which only other workgroups on the same CU cover, so the number of
workgroups a CU holds is what its time hangs on (its comment: three per CU 2.03 ms, four 1.85 ms on the 64 GiB tree).  The comment
states four: 4 x 8 waves are 8 per SIMD, 512 registers / 8 = 64 a wave, and four times its LDS must fit a CU's 160 KiB.  Scratch or
AGPRs would meet the register number by moving values, not by needing fewer.

Compiled as tests/test_k3_leaf_budget.py does: for gfx950 with the flags the Makefile gives the product library, device code only."""
import re
import subprocess

import pytest

from tests.test_k3_leaf_budget import ROOT, SRC, hipcc, product_flags, summaries

WORKGROUPS_PER_CU = 4
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512


@pytest.fixture(scope="module")
def parents_kernel(tmp_path_factory):
    cc = hipcc()
    if cc is None:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("k3p") / "k_blake3.s"
    cmd = [cc] + product_flags() + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", str(SRC), "-o", str(out)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    found = {k: v for k, v in summaries(res.stderr).items() if "k_blake3_parents_window" in k}
    assert len(found) == 1, sorted(found)  # the product has one small-tree reducer, no switch
    return next(iter(found.values()))


def test_comment_states_the_workgroups_per_cu():
    text = SRC.read_text()
    assert re.search(r"FOUR workgroups are resident per CU", text) and re.search(r"FOUR workgroups per CU", text)


def test_parents_kernel_fits_four_workgroups_per_cu(parents_kernel):
    k = parents_kernel
    print(k)
    threads = int(re.search(r"^constexpr int PW_THREADS = (\d+);", SRC.read_text(), re.M).group(1))
    waves_per_simd = WORKGROUPS_PER_CU * (threads // 64) / 4
    assert waves_per_simd <= 8, f"{WORKGROUPS_PER_CU} workgroups of {threads} threads are {waves_per_simd} waves per SIMD, a SIMD holds 8"
    budget = VGPRS_PER_SIMD // int(waves_per_simd)
    assert k["ScratchSize"] == 0, f"{k['ScratchSize']} bytes of scratch per lane"
    assert k["AGPRs"] == 0, f"{k['AGPRs']} AGPRs"
    assert k["VGPRs"] <= budget, f"{k['VGPRs']} VGPRs, budget {budget} for {WORKGROUPS_PER_CU} workgroups per CU"
    assert k["Occupancy"] >= waves_per_simd, k
    assert WORKGROUPS_PER_CU * k["LDS Size"] <= LDS_PER_CU, f"{k['LDS Size']} bytes of LDS per workgroup: {LDS_PER_CU // k['LDS Size']} per CU"
