"""CPU-only: the host code of the archive index (longtail_amd/csrc/archive_layout.h over restore_parse.h) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program (tests/san/archive_driver.cpp, its own main)
includes it alone, is compiled with -fsanitize=address,undefined and run as a program -- nothing is preloaded.  Every buffer the header
sees lies at an ODD address, so that a load through a typed pointer is reported; the u64 table of the index is 4-byte aligned in one case
and 8-byte aligned in the other.  The index the program writes must be lthip_archive_write_index's, what it opens must be what was
written, every proper prefix, an over-long index, huge counts and offset + size overflows must come back EBADF, and the merged ranges
must be the Python model's -- all without a sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from longtail_amd.lib import archive_write_index
from tests.test_archive_abi import LZ4, indexes

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "archive_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
RANGES = [(100, 10), (0, 10), (10, 5), (120, 1), (105, 30), (2**64 - 5, 4), (200, 0)]


def merged(ranges, gap):
    out = []
    for first, n in sorted(ranges):
        if out and first - (out[-1][0] + out[-1][1]) <= gap:
            out[-1][1] = max(out[-1][0] + out[-1][1], first + n) - out[-1][0]
        else:
            out.append([first, n])
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("archive")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "archive_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


@pytest.mark.parametrize("nb,per_block,path_len", [(3, 2, 3), (2, 2, 6), (0, 0, 1)])
def test_write_open_prefixes_and_overflows_without_a_sanitizer_report(hiplib, driver, nb, per_block, path_len):
    exe, out = driver
    si, vi, sizes = indexes(nb, per_block, path_len, tags=[LZ4 if b % 2 else 0 for b in range(nb)])
    offsets = np.array([4001 - 1333 * b for b in range(nb)], np.uint64)  # descending, odd and even
    (out / "si.bin").write_bytes(si)
    (out / "vi.bin").write_bytes(vi)
    (out / "t.bin").write_bytes(offsets.tobytes() + np.array(sizes, np.uint32).tobytes())
    run = subprocess.run([str(exe), str(out / "si.bin"), str(out / "vi.bin"), str(out / "t.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    index = archive_write_index(si, vi, offsets, sizes)
    assert lines[0] == "index " + index.hex()
    end = max([int(o) + z for o, z in zip(offsets, sizes)], default=0)
    opened = " ".join(str(x) for x in [nb, end, *[int(o) for o in offsets], *sizes])
    assert lines[1] == lines[2] == "open " + opened
    for k, gap in enumerate((0, 9, 2**64 - 1)):
        assert lines[3 + k] == f"ranges {gap}:" + "".join(f" {a}+{n}" for a, n in merged(RANGES, gap))
    assert lines[-1] == f"ok {2 + (1 if nb else 0) + len(index) + 1 + 5 * 11 + 2 * nb + 3}"
