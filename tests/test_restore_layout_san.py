"""CPU-only: lthip_restore_layout_in_place's host code (longtail_amd/csrc/restore_layout.h over version_diff.h and restore_parse.h) under
AddressSanitizer and UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program
(tests/san/restore_layout_driver.cpp, its own main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program
-- nothing is preloaded.  It lays out the hand-built versions of tests/test_restore_in_place_abi.py (the offsets must be the Python
model's) and offers every proper prefix of either blob: all must come back EBADF, without a sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.test_restore_in_place_abi import BASE, CASES, dense, model, version

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "restore_layout_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("restore_layout")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "restore_layout_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


@pytest.mark.parametrize("align", [1, 4096])
@pytest.mark.parametrize("case", list(CASES))
def test_the_offsets_and_every_prefix_without_a_sanitizer_report(driver, case, align):
    exe, out = driver
    c = CASES[case]
    base_offsets, base_bytes = dense(BASE, skip=c.get("skip", ()))
    a, b = version(BASE), version(c["target"])
    (out / "a.bin").write_bytes(a)
    (out / "b.bin").write_bytes(b)
    (out / "o.bin").write_bytes(np.array(base_offsets, np.uint64).tobytes())
    run = subprocess.run([str(exe), str(out / "a.bin"), str(out / "b.bin"), str(out / "o.bin"), str(base_bytes), str(align)],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines[:3]}
    want = model(BASE, base_offsets, base_bytes, c["target"], align)
    assert got == {"offsets": want[0], "total": [want[1]], "kept": [want[2]]}
    assert lines[-1] == f"ok {2 + len(a) + len(b) + 5}"
