"""CPU-only: the host code of the store index operations (longtail_amd/csrc/store_index_ops.h over restore_parse.h) under
AddressSanitizer and UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program
(tests/san/store_index_ops_driver.cpp, its own main) includes it alone, is compiled with -fsanitize=address,undefined and run as a
program -- nothing is preloaded.  Every blob the header reads and every output it writes lies at an ODD address and ends where its
allocation ends, so that a load or store through a typed pointer, or one byte past a blob, is reported.  What the program prunes and
merges must be what the library's entry points give (which tests/test_store_index_ops_abi.py holds against the reference), every proper
prefix and every wrapping head word must come back EBADF -- all without a sanitizer report."""
import errno
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from longtail_amd.lib import LongtailHipError, store_index_merge, store_index_prune, version_chunk_hashes
from tests.restore_util import BLK3, build_version_index
from tests.store_index_ops_util import A, B, EMPTY, HASHES, NO_CHUNKS, ONES, OTHER_HASH, SIZES, TWICE, TWICE_REMOTE

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "store_index_ops_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
VI = build_version_index(BLK3, 4096, ["a.bin", "dir/", "dir/b.bin"], [[0, 1, 2, 1], [], [3, 0, 4]], HASHES[:5], SIZES[:5])
NO_CHUNKS_VI = build_version_index(BLK3, 4096, ["dir/"], [[]], HASHES[:0], SIZES[:0])
CASES = {
    "a block on both sides": (A, B, [ONES, 0xA3, 0x77, 0xA3, 0xA1], VI),
    "block hashes that stand twice": (TWICE, TWICE_REMOTE, [0xD1], VI),
    "conflicting identifiers": (A, OTHER_HASH, [], VI),
    "an empty local": (EMPTY, A, [5], NO_CHUNKS_VI),
    "blocks without chunks": (NO_CHUNKS, EMPTY, [0xE1, 0xE2], VI),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("store_index_ops")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "store_index_ops_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


def merged_line(name, local, remote):
    try:
        return f"{name} " + store_index_merge(local, remote).hex()
    except LongtailHipError as e:
        assert e.code == errno.EINVAL
        return f"{name} errno {errno.EINVAL}"


@pytest.mark.parametrize("case", list(CASES))
def test_prune_merge_prefixes_and_overflows_without_a_sanitizer_report(hiplib, driver, case):
    exe, out = driver
    local, remote, keep, vi = CASES[case]
    for name, blob in (("local", local), ("remote", remote), ("keep", np.array(keep, np.uint64).tobytes()), ("vi", vi)):
        (out / f"{name}.bin").write_bytes(blob)
    run = subprocess.run([str(exe), *[str(out / f"{n}.bin") for n in ("local", "remote", "keep", "vi")]], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    assert lines[0] == "prune " + store_index_prune(local, keep).hex()
    assert lines[1] == merged_line("merge", local, remote) and lines[2] == merged_line("merge_rev", remote, local)
    hashes = version_chunk_hashes(vi)
    assert lines[3] == " ".join(["hashes", str(len(hashes)), *[str(int(h)) for h in hashes]])
    refused = lines[1].startswith("merge errno")
    nb = int(np.frombuffer(local[8:12], np.uint32)[0])
    assert lines[-1] == f"ok {3 + 2 * (1 if refused else 3) + 3 + len(local) + len(vi) + 5 * 4 + (1 if nb else 0)}"
