"""CPU-only: lthip_version_diff's host code (longtail_amd/csrc/version_diff.h over restore_parse.h) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program (tests/san/version_diff_driver.cpp, its own
main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program -- nothing is preloaded.  It diffs the
hand-built versions of tests/test_restore_update_abi.py (the lists must be the ones written out there) and offers every proper prefix of
either blob: all must come back EBADF, without a sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import pytest

from tests.test_restore_update_abi import CASES, KEYS, expected_of, version

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "version_diff_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("version_diff")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "version_diff_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


@pytest.mark.parametrize("case", ["hand", "reversed", "empty source"])
def test_the_lists_and_every_prefix_without_a_sanitizer_report(driver, case):
    exe, out = driver
    src, tgt = CASES[case]
    a, b = version(src), version(tgt)
    (out / "a.bin").write_bytes(a)
    (out / "b.bin").write_bytes(b)
    run = subprocess.run([str(exe), str(out / "a.bin"), str(out / "b.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines[:6]}
    assert got == {k: expected_of(case)[k] for k in KEYS}
    assert lines[-1] == f"ok {1 + len(a) + len(b)}"
