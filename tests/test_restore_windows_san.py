"""CPU-only: the host code of the window restore (longtail_amd/csrc/restore_windows.h over restore_parse.h) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program (tests/san/restore_windows_driver.cpp, its own
main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program -- nothing is preloaded.  It expands the
windows of the clip sweep of tests/test_gpu_restore_windows.py on the hand-built VersionIndex (the occurrence table must be the Python
model's, tests/restore_windows_util.py), a set of whole-asset and zero-length windows, every invalid window alone, 32 768 windows over an
asset of 65 536 chunks (one occurrence too many for a session, refused before anything is allocated), and offers every proper prefix of
the blob: all must come back EBADF, without a sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from longtail_amd.lib import RESTORE_WINDOW_DTYPE, _window_table
from tests.restore_util import BLK3, build_version_index
from tests.restore_windows_util import LENGTHS, SWEEP_ASSETS, model_occurrences, sweep_version, sweep_windows

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "restore_windows_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
HASHES = [1000 + 7 * k for k in range(len(LENGTHS))]
SIZES = [sum(LENGTHS[c] for c in cs) for cs in SWEEP_ASSETS]
M = 2**64


def invalid_windows(out_bytes):
    """Raw (asset, reserved, offset, length, dst) records, each invalid on its own for the sweep's version."""
    return [(len(SIZES), 0, 0, 0, 0), (0xFFFFFFFF, 0, 0, 1, 0), (0, 1, 0, 1, 0), (0, 0, SIZES[0], 1, 0), (0, 0, SIZES[0] + 1, 0, 0),
            (1, 0, 1, SIZES[1], 0), (1, 0, 2, M - 1, 0), (1, 0, M - 1, 2, 0), (0, 0, 0, 2, out_bytes - 1), (0, 0, 0, 0, out_bytes + 1),
            (2, 0, 0, 2, M - 1), (2, 0, 5, 1, M - 1)]


def raw_table(records):
    t = np.zeros(len(records), RESTORE_WINDOW_DTYPE)
    for i, r in enumerate(records):
        t[i] = r
    return t


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("restore_windows")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "restore_windows_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


def run(driver, vi, windows, out_bytes, extra=()):
    exe, out = driver
    (out / "vi.bin").write_bytes(vi)
    (out / "w.bin").write_bytes(_window_table(windows).tobytes())
    bad = invalid_windows(out_bytes)
    (out / "bad.bin").write_bytes(raw_table(bad).tobytes())
    got = subprocess.run([str(exe), str(out / "vi.bin"), str(out / "w.bin"), str(out / "bad.bin"), str(out_bytes), *extra], capture_output=True,
                         text=True, timeout=300)
    assert got.returncode == 0, (got.stdout[-2000:], got.stderr[-4000:])
    assert "ERROR" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    lines = got.stdout.splitlines()
    occ, selected = model_occurrences(vi, windows)
    assert lines[0] == f"selected {selected}"
    assert [tuple(int(x) for x in ln.split()) for ln in lines[1 : 1 + len(occ)]] == occ
    assert lines[1 + len(occ)] == "sizes " + " ".join(str(s) for s in SIZES) and lines[2 + len(occ)] == "target 32768"
    assert lines[-1] == f"ok {2 + len(bad) + 1 + len(vi) + (1 if extra else 0)}"
    return occ


def test_the_sweeps_occurrences_and_every_prefix_without_a_sanitizer_report(driver):
    vi, _ = sweep_version(HASHES)
    windows, out_bytes = sweep_windows()
    occ = run(driver, vi, windows, out_bytes)
    assert len(occ) > len(windows) > 200 and any(s and c < n - s for _, n, s, c, _ in occ)
    assert {d % 16 for *_, d in occ} == set(range(16))


def test_whole_assets_zero_lengths_and_too_many_occurrences(driver):
    exe, out = driver
    vi, _ = sweep_version(HASHES)
    windows = [(a, 0, n, 100 + 5000 * a) for a, n in enumerate(SIZES)] + [(1, 7, 0, 3), (2, SIZES[2], 0, 20000), (0, 0, SIZES[0], 0)]
    # one asset of 65 536 one-byte chunks: 32 768 whole windows are 2^31 occurrences
    n = 65536
    big = build_version_index(BLK3, 32768, ["big"], [list(range(n))], np.arange(1, n + 1, dtype=np.uint64), np.ones(n, np.uint32))
    (out / "big.bin").write_bytes(big)
    occ = run(driver, vi, windows, 20000, extra=(str(out / "big.bin"), "32768"))
    assert all(s == 0 and c == n for _, n, s, c, _ in occ) and len(occ) == len(SWEEP_ASSETS[0]) * 2 + len(SWEEP_ASSETS[1]) + len(SWEEP_ASSETS[2])
