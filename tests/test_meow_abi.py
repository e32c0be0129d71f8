"""CPU-only checks of the 'meow' hash type: the Meow entry points are declared and exported by both builds, the gfx950 code object
holds the Meow kernels, the constructor and bulk calls refuse cleanly without a GPU, the project's CPU model of Meow (tests/meow_model.py)
matches the digests the reference produced (tests/golden/meow_vectors.json), and the kernel's seed is π in hexadecimal."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.meow_model import SEED, meow, meow_batch, pi_hex_digits
from tests.test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "meow_vectors.json").read_text())

MEOW_SYMBOLS = ["Longtail_CreateHipMeowHashAPI", "lthip_meow_ranges", "lthip_meow_ranges_dev", "lthip_meow_one", "lthip_meow_runs_u64",
                "lthip_meow_runs_u64_bounded", "lthip_meow_stream_batch", "lthip_meow_stream_final"]
MEOW_KERNELS = ["k_meow_lanes", "k_meow_quads", "k_meow_one", "k_meow_stream"]


def xorshift_from(seed: int, nbytes: int) -> np.ndarray:
    """SURVEY.md §8(c)'s xorshift64 stream started from `seed` (the state after each step as 8 little-endian bytes)"""
    words = (nbytes + 7) // 8
    out = np.empty(words, np.uint64)
    s, mask = seed, (1 << 64) - 1
    for i in range(words):
        s ^= (s << 13) & mask
        s ^= s >> 7
        s ^= (s << 17) & mask
        out[i] = s
    return out.view(np.uint8)[:nbytes]


def golden_input(v) -> np.ndarray:
    return xorshift_from(v["seed"], v["offset"] + v["len"])[v["offset"] :]


def test_meow_entry_points_are_declared_and_exported(hiplib):
    declared = declared_symbols()
    assert set(MEOW_SYMBOLS) <= set(declared)
    missing = [n for n in MEOW_SYMBOLS if not hasattr(hiplib.dll, n)]
    assert not missing, missing
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in MEOW_SYMBOLS if not hasattr(abl, n)]


def test_code_object_holds_the_meow_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in MEOW_KERNELS:
        assert k in text, k
    assert "amdgcn-amd-amdhsa--gfx950" in text


def test_meow_constants_and_kernel_ids_are_unchanged():
    from longtail_amd import lib

    h = (ROOT / "include" / "longtail_hip.h").read_text()
    assert int(re.search(r"LTHIP_K_COUNT = (\d+)", h).group(1)) == 11
    assert re.search(r"#define LTHIP_MEOW_STREAM_BATCH LTHIP_B3_STREAM_BATCH", h) and lib.MEOW_STREAM_BATCH == 1 << 20
    assert int(re.search(r"#define LTHIP_MEOW_STREAM_STATE_BYTES (\d+)u", h).group(1)) == lib.MEOW_STREAM_STATE_BYTES
    assert lib.HASH_MEOW == 0x6D656F77 == int.from_bytes(b"meow", "big")
    assert "0x6d656f77u" in (ROOT / "longtail_amd" / "csrc" / "lthip_internal.h").read_text()


def test_meow_constructor_refuses_without_a_gpu(hiplib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("this check is for a machine without a GPU (tests/test_gpu_meow.py covers the object)")
    d = hiplib.dll
    assert not d.Longtail_CreateHipMeowHashAPI()
    # the bulk calls validate their arguments before they touch a device
    assert d.lthip_meow_one(None, None, 0, None) != 0
    assert d.lthip_meow_ranges(None, None, 1, None, None, 0, None) != 0
    assert d.lthip_meow_ranges_dev(None, None, 1, None, None, None, 0, None) != 0
    assert d.lthip_meow_runs_u64(None, None, None, 1, None) != 0
    assert d.lthip_meow_runs_u64_bounded(None, None, None, 1, 0, 0, None) != 0
    assert d.lthip_meow_stream_batch(None, None, 0, None) != 0
    assert d.lthip_meow_stream_final(None, None, 0, 0, None, None) != 0


def test_seed_of_the_kernel_is_pi_in_hex():
    src = (ROOT / "longtail_amd" / "csrc" / "k_meow.hip").read_text()
    body = re.search(r"MEOW_SEED_PI\[32\] = \{(.*?)\};", src, re.S).group(1)
    words = re.findall(r"0x([0-9A-Fa-f]{8})", body)
    assert len(words) == 32
    assert "".join(words).upper() == pi_hex_digits(256)
    assert SEED[:8].hex().upper() == "3243F6A8885A308D" and SEED[-4:].hex().upper() == "871574E6"


def test_model_matches_the_reference_digests():
    for v in GOLDEN["vectors"]:
        assert meow(golden_input(v)) == int(v["digest"], 16), (v["len"], v["offset"], v["seed"])
    st = GOLDEN["stream"]
    assert meow(golden_input(st)) == int(st["digest"], 16)


def test_model_batch_equals_single_messages():
    rng = np.random.default_rng(1)
    lens = np.array([0, 1, 31, 32, 255, 256, 257, 700, 1000, 513], np.int64)
    data = rng.integers(0, 256, size=(len(lens), 1024), dtype=np.uint8)
    got = meow_batch(data, lens)
    assert [int(g) for g in got] == [meow(data[i, : lens[i]]) for i in range(len(lens))]
