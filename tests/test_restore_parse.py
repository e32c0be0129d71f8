"""CPU-only: the blob parsing of the restore session (longtail_amd/csrc/restore_parse.h) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program (tests/san/restore_parse_driver.cpp, its own
main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program -- nothing is preloaded.  It feeds the parser
every proper prefix of a valid VersionIndex and of a valid StoreIndex, each header word set to 0xFFFFFFFF and counts that overflow the
size arithmetic: all must come back EBADF, the valid blob 0, without a sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.restore_util import BLK3, build_store_index, build_version_index

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "restore_parse_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("restore_parse")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "restore_parse_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


def blobs():
    rng = np.random.default_rng(3)
    sizes = [1, 2, 3, 4, 5, 15, 16, 17, 4097]
    hashes = rng.integers(1, 2**63, len(sizes)).astype(np.uint64)
    names = ["d/", "d/empty", "d/a", "d/b", "e/c"]
    chunks = [[], [], [0, 1, 2, 8], [8, 3, 4], [5, 6, 7, 0]]
    vi = build_version_index(BLK3, 32768, names, chunks, hashes, sizes)
    si = build_store_index(BLK3, [(11, 0, [0, 1, 2]), (12, 0x6C7A3432, [3, 4, 5, 6]), (13, 0x7A746432, [7, 8])], hashes, sizes)
    return vi, si


@pytest.mark.parametrize("kind", ["vi", "si"])
def test_malformed_blobs_are_ebadf_without_a_sanitizer_report(driver, kind):
    exe, out = driver
    vi, si = blobs()
    blob = vi if kind == "vi" else si
    path = out / f"{kind}.bin"
    path.write_bytes(blob)
    run = subprocess.run([str(exe), kind, str(path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    words = 6 if kind == "vi" else 4
    cases = int(run.stdout.split()[-1])
    assert run.stdout.startswith("ok ") and cases >= len(blob) + words + 6, run.stdout
