"""The register budget of the BLAKE3 leaf pass, read from the compiler's resource summary of k_blake3.hip (no GPU).

k_blake3_leaves is bound by vector instruction issue and runs eight waves per SIMD, the most there are: 512 registers / 8 = 64 a wave.
It keeps two sets of 17 message dwords (the block being compressed and the next one's loads in flight), 16 state words and the
message in the first set's registers; one register more than 64 costs a wave per SIMD, which DESIGN.md §3 measured at +4 % time for
four.  Scratch or AGPRs would meet the number by moving values, not by needing fewer.

The file is compiled for gfx950 with the flags the Makefile gives the product library (no -DLTHIP_ABLATIONS), device code only, and the
numbers are those of `-Rpass-analysis=kernel-resource-usage`."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "longtail_amd" / "csrc" / "k_blake3.hip"
VGPR_BUDGET = 64


def hipcc():
    if os.environ.get("HIPCC"):
        return os.environ["HIPCC"]
    for r in [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]:
        if r and (Path(r) / "bin" / "hipcc").exists():
            return str(Path(r) / "bin" / "hipcc")
    return shutil.which("hipcc")


def product_flags():
    """HIPFLAGS of the Makefile with ARCH filled in, without the dependency-file switches and the (empty by default) extras."""
    mk = (ROOT / "Makefile").read_text()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    return [f.replace("$(ARCH)", arch) for f in flags if f not in ("-MMD", "-MP", "$(EXTRA_HIPFLAGS)")]


def summaries(text):
    """kernel name -> {field: int} from the remarks of -Rpass-analysis=kernel-resource-usage."""
    found, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: \s*(.+?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        key, val = m.group(1).split(" [")[0].strip(), m.group(2)  # ("ScratchSize [bytes/lane]" -> "ScratchSize")
        if key == "Function Name":
            cur = found.setdefault(val, {})
        elif cur is not None and val.isdigit():
            cur[key] = int(val)
    return found


@pytest.fixture(scope="module")
def leaf_kernels(tmp_path_factory):
    cc = hipcc()
    if cc is None:
        pytest.skip("hipcc not found")
    out = tmp_path_factory.mktemp("k3") / "k_blake3.s"
    cmd = [cc] + product_flags() + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", str(SRC), "-o", str(out)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return {k: v for k, v in summaries(res.stderr).items() if "k_blake3_leaves" in k}


def test_product_flags_are_the_makefiles():
    flags = product_flags()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags and "-DLTHIP_ABLATIONS" not in flags, flags


def test_leaf_pass_keeps_eight_waves_per_simd(leaf_kernels):
    assert len(leaf_kernels) == 1, sorted(leaf_kernels)  # the product has one form of the kernel, no switch
    for name, k in leaf_kernels.items():
        print(f"{name}: {k}")
        assert k["VGPRs"] <= VGPR_BUDGET, f"{name}: {k['VGPRs']} VGPRs, budget {VGPR_BUDGET}"
        assert k["AGPRs"] == 0, f"{name}: {k['AGPRs']} AGPRs"
        assert k["ScratchSize"] == 0, f"{name}: {k['ScratchSize']} bytes of scratch per lane"
