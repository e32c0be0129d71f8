"""The register budget of the walking scan that hashes (k_buzhash_hash_walk), read from the kernel metadata of the built library (no GPU).

The kernel runs one 16-wave workgroup per CU, four waves per SIMD, like k_buzhash_walk: the BLAKE3 leaf body (63 registers, no LDS) has
to fit inside the walk's allocation, so that on every SIMD some of the four waves scan while the others hash.  At more than 104
registers the kernel would still run at four waves (the launch bounds give it 128), but the budget is the one the walking scan keeps
(tests/test_k1_walk_budget.py), and scratch or AGPRs would meet it by moving values, not by needing fewer."""
import re
import subprocess

import pytest

from tests.test_k1_walk_budget import ABL, LIB, VGPR_BUDGET, code_objects, kernels_of, readelf

NAME = "k_buzhash_hash_walk"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tool = readelf()
    if tool is None:
        pytest.skip("llvm-readelf not found")
    assert LIB.exists(), f"{LIB} is missing: run make (or __graft_entry__.build())"
    d = tmp_path_factory.mktemp("co")
    found = {}
    for lib in [LIB] + ([ABL] if ABL.exists() else []):
        tag = lib.parent.name
        for i, o in enumerate(code_objects(lib.read_bytes())):
            if NAME.encode() not in o:
                continue
            f = d / f"{tag}{i}.elf"
            f.write_bytes(o)
            notes = subprocess.run([tool, "--notes", str(f)], check=True, capture_output=True, text=True).stdout
            found.update({f"{tag}: {k}": v for k, v in kernels_of(notes).items() if NAME in k})
    return found


def test_both_modes_are_built(kernels):
    modes = {re.search(NAME + r"ILi(\d)ELi16ELb([01])E", k).groups() for k in kernels if k.startswith("longtail_amd: ")}
    assert {m for m, _ in modes} == {"0", "1"}, sorted(kernels)


def test_hashing_walk_fits_the_walks_allocation(kernels):
    assert kernels
    for name, k in sorted(kernels.items()):
        vgpr, agpr, scratch = int(k[".vgpr_count"]), int(k[".agpr_count"]), int(k[".private_segment_fixed_size"])
        print(f"{name}: vgpr {vgpr} agpr {agpr} scratch {scratch}")
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs, budget {VGPR_BUDGET}"
        assert agpr == 0, f"{name}: {agpr} AGPRs"
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
