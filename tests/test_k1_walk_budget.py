"""The register budget of the walking scan, read from the kernel metadata of the built library (no GPU).

k_buzhash_walk runs one 16-wave workgroup per CU: four waves per SIMD.  The sliced pass of lthip_chunk_hash runs the scan of slice
k + 1 beside the BLAKE3 leaf hashing of slice k, and a leaf wave (48 registers allocated) finds room on a SIMD only if the four scan
waves leave it there: at <= 104 registers each they leave 96 of the 512, two leaf waves; at the 128 of the launch bounds they leave
none and the two passes run one after the other.  Scratch and AGPRs would meet the number by moving values, not by
needing fewer.

The numbers are the `.vgpr_count`, `.agpr_count` and `.private_segment_fixed_size` entries of the code objects' notes, as
`llvm-readelf --notes` prints them."""
import os
import re
import shutil
import struct
import subprocess
from pathlib import Path

import pytest

LIB = Path(__file__).resolve().parent.parent / "longtail_amd" / "liblongtail_hip.so"
ABL = LIB.parent.parent / "build" / "ablations" / "liblongtail_hip.so"  # (when built: it holds the other prefetch form, GUESS = 0, as well)
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
VGPR_BUDGET = 104


def readelf():
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]
    for r in roots:
        if r and (Path(r) / "llvm" / "bin" / "llvm-readelf").exists():
            return str(Path(r) / "llvm" / "bin" / "llvm-readelf")
    return shutil.which("llvm-readelf")


def code_objects(blob):
    """The gfx code objects of every offload bundle in a host library (one bundle per translation unit)."""
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24 : p + 24 + tlen].decode()
            p += 24 + tlen
            if "amdgcn" in triple and size:
                out.append(blob[at + off : at + off + size])
        at = blob.find(MAGIC, at + len(MAGIC))
    return out


def kernels_of(notes):
    """name -> {key: value} of the amdhsa.kernels entries in the text of `llvm-readelf --notes`."""
    found, cur = {}, None
    for line in notes.splitlines():
        first = re.match(r"^  - (\.\w+):\s*(.*)$", line)
        m = first or re.match(r"^    (\.\w+):\s*(.*)$", line)
        if first:
            cur = {}
        if m and cur is not None:
            cur[m.group(1)] = m.group(2).strip().strip("'\"")
            if m.group(1) == ".name":
                found[cur[".name"]] = cur
        elif not line.startswith("      "):  # (deeper lines are the kernel's argument list; anything else ends the list of kernels)
            cur = None
    return found


@pytest.fixture(scope="module")
def walk_kernels(tmp_path_factory):
    tool = readelf()
    if tool is None:
        pytest.skip("llvm-readelf not found")
    assert LIB.exists(), f"{LIB} is missing: run make (or __graft_entry__.build())"
    d = tmp_path_factory.mktemp("co")
    walk = {}
    for lib in [LIB] + ([ABL] if ABL.exists() else []):
        objs = code_objects(lib.read_bytes())
        assert objs, f"no gfx code object found in the offload bundles of {lib}"
        tag = lib.parent.name
        for i, o in enumerate(objs):
            if b"k_buzhash_walk" not in o:
                continue
            f = d / f"{tag}{i}.elf"
            f.write_bytes(o)
            notes = subprocess.run([tool, "--notes", str(f)], check=True, capture_output=True, text=True).stdout
            walk.update({f"{tag}: {k}": v for k, v in kernels_of(notes).items() if "k_buzhash_walk" in k})
    return walk


def test_both_modes_are_built(walk_kernels):
    # k_buzhash_walk<MODE, 16, GUESS>: the divisor test (MODE 0) and the power-of-two test (MODE 1) of the product's prefetch form
    modes = {re.search(r"k_buzhash_walkILi(\d)ELi16ELb([01])E", k).groups() for k in walk_kernels if k.startswith("longtail_amd: ")}
    assert {m for m, _ in modes} == {"0", "1"}, sorted(walk_kernels)


def test_walking_scan_leaves_room_for_two_leaf_waves(walk_kernels):
    assert walk_kernels
    for name, k in sorted(walk_kernels.items()):
        vgpr, agpr, scratch = int(k[".vgpr_count"]), int(k[".agpr_count"]), int(k[".private_segment_fixed_size"])
        print(f"{name}: vgpr {vgpr} agpr {agpr} scratch {scratch}")
        assert vgpr <= VGPR_BUDGET, f"{name}: {vgpr} VGPRs, budget {VGPR_BUDGET}"
        assert agpr == 0, f"{name}: {agpr} AGPRs"
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
