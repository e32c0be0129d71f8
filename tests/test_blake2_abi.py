"""CPU-only checks of the 'blk2' hash type: the BLAKE2s entry points are declared and exported by both builds, the gfx950 code object
holds the BLAKE2s kernels, and the kernel-timing id sits behind its own accessor (bench.py's per-kernel dict is unchanged)."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from tests.test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent

B2_SYMBOLS = ["Longtail_CreateHipBlake2HashAPI", "lthip_blake2s_ranges", "lthip_blake2s_ranges_dev", "lthip_blake2s_one",
              "lthip_blake2s_runs_u64", "lthip_blake2s_runs_u64_bounded", "lthip_b2s_stream_batch", "lthip_b2s_stream_final"]
B2_KERNELS = ["k_b2s_lanes", "k_b2s_quads", "k_b2s_one", "k_b2s_stream", "k_b2s_class_hist", "k_b2s_class_scatter"]


def test_blake2_entry_points_are_declared_and_exported(hiplib):
    declared = declared_symbols()
    assert set(B2_SYMBOLS) <= set(declared)
    missing = [n for n in B2_SYMBOLS if not hasattr(hiplib.dll, n)]
    assert not missing, missing
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in B2_SYMBOLS if not hasattr(abl, n)]


def test_code_object_holds_the_blake2s_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in B2_KERNELS:
        assert k in text, k
    assert "amdgcn-amd-amdhsa--gfx950" in text


def test_blake2s_kernel_id_is_appended_and_kept_out_of_the_bench_dict():
    from longtail_amd import lib

    h = (ROOT / "include" / "longtail_hip.h").read_text()
    assert int(re.search(r"LTHIP_K_GATHER = (\d+)", h).group(1)) == 9
    assert int(re.search(r"LTHIP_K_BLAKE2S = (\d+)", h).group(1)) == lib.BLAKE2S_KERNEL_ID == 10
    assert int(re.search(r"LTHIP_K_COUNT = (\d+)", h).group(1)) == 11
    assert lib.BLAKE2S_KERNEL_ID not in lib.KERNEL_IDS.values() and len(lib.KERNEL_IDS) == 10
    assert int(re.search(r"#define LTHIP_B2S_STREAM_BATCH \(1u << (\d+)\)", h).group(1)) == 20 and lib.B2S_STREAM_BATCH == 1 << 20
    assert int(re.search(r"#define LTHIP_B2S_STREAM_STATE_BYTES (\d+)u", h).group(1)) == lib.B2S_STREAM_STATE_BYTES


def test_blake2_constructor_refuses_without_a_gpu(hiplib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("this check is for a machine without a GPU (tests/test_gpu_blake2.py covers the object)")
    d = hiplib.dll
    assert not d.Longtail_CreateHipBlake2HashAPI()
    # the bulk calls validate their arguments before they touch a device
    assert d.lthip_blake2s_one(None, None, 0, None) != 0
    assert d.lthip_blake2s_ranges(None, None, 1, None, None, 0, None) != 0
    assert d.lthip_blake2s_ranges_dev(None, None, 1, None, None, None, 0, None) != 0
    assert d.lthip_blake2s_runs_u64(None, None, None, 1, None) != 0
    assert d.lthip_blake2s_runs_u64_bounded(None, None, None, 1, 0, 0, None) != 0
    assert d.lthip_b2s_stream_batch(None, None, 0, None) != 0
    assert d.lthip_b2s_stream_final(None, None, 0, 0, None, None) != 0
