"""CPU-only: the host tables of the restore session's plan (longtail_amd/csrc/restore_plan.h over restore_parse.h and restore_windows.h)
under AddressSanitizer and UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program
(tests/san/restore_plan_driver.cpp, its own main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program
-- nothing is preloaded.  Its tables must be those of the numpy models below, its refusals the library's errno and message, and no run
may leave a sanitizer report."""
import errno
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.restore_util import BLK3, STORE_INDEX_VERSION, build_store_index, build_version_index, parse_store_index, parse_version_index
from tests.restore_windows_util import LENGTHS, SWEEP_ASSETS, sweep_version

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "restore_plan_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NONE, NOWHERE, SKIP = 0xFFFFFFFF, 2**64 - 1, 2**64 - 1
HASHES = [1000 + c for c in range(len(LENGTHS))]
LEAVES_BASE = "a resident asset's window leaves the base"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("restore_plan")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "restore_plan_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


def run(driver, mode, index, offsets=None, *more):
    """-> the driver's output lines; the run must end with status 0 and without a sanitizer report."""
    exe, out = driver
    (out / "index.bin").write_bytes(index)
    args = [str(exe), mode, str(out / "index.bin")]
    if offsets is not None:
        (out / "offsets.bin").write_bytes(np.array(offsets, np.uint64).tobytes())
        args.append(str(out / "offsets.bin"))
    got = subprocess.run(args + [str(m) for m in more], capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, (got.stdout[-2000:], got.stderr[-4000:])
    assert "ERROR" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    return got.stdout.splitlines()


def tables(lines):
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines}


# ---- store_tables ----


def model_store_tables(si):
    p = parse_store_index(si)
    m, sizes = len(p["chunk_sizes"]), p["chunk_sizes"].astype(np.int64)
    cblock, coff = np.full(m, NONE, np.int64), np.zeros(m, np.int64)
    braw, bleaves = [], []
    for b, (first, count) in enumerate(zip(p["block_offsets"].tolist(), p["block_counts"].tolist())):
        mine = sizes[first : first + count]
        local = np.concatenate([[0], np.cumsum(mine)])  # block-local prefix sums
        for k in range(count):
            if cblock[first + k] == NONE:  # the first block that lists a position keeps it
                cblock[first + k], coff[first + k] = b, local[k]
        braw.append(int(local[-1]))
        bleaves.append(int(np.maximum(1, (mine + 1023) // 1024).sum()))
    return dict(max_chunk=[int(sizes.max()) if m else 0], block_chunks=[int(p["block_counts"].sum())], chash=p["chunk_hashes"].tolist(),
                csize=sizes.tolist(), cblock=cblock.tolist(), coff=coff.tolist(), bhash=p["block_hashes"].tolist(),
                bcoff=p["block_offsets"].tolist(), bcnt=p["block_counts"].tolist(), btag=p["block_tags"].tolist(), braw=braw, bleaves=bleaves)


def shared_position_index():
    """The sweep's StoreIndex with its blocks moved so that chunk position 2 is listed by block 0 (positions 0..2) and by block 1
    (positions 2..3); block 2 lists 4..6.  No writer produces such an index; the parser accepts it."""
    p = parse_store_index(sweep_version(HASHES)[1])
    head = np.array([STORE_INDEX_VERSION, BLK3, 3, len(LENGTHS)], np.uint32)
    return b"".join([head.tobytes(), p["block_hashes"].tobytes(), p["chunk_hashes"].tobytes(), np.array([0, 2, 4], np.uint32).tobytes(),
                     np.array([3, 2, 3], np.uint32).tobytes(), p["block_tags"].tobytes(), p["chunk_sizes"].tobytes()])


@pytest.mark.parametrize("which", ["sweep", "shared position", "empty"])
def test_store_tables_are_the_models(driver, which):
    si = {"sweep": lambda: sweep_version(HASHES)[1], "shared position": shared_position_index,
          "empty": lambda: build_store_index(BLK3, [], np.zeros(0, np.uint64), np.zeros(0, np.uint32))}[which]()
    want = model_store_tables(si)
    if which == "sweep":
        assert want["cblock"] == [0, 0, 0, 1, 1, 2, 2] and want["coff"] == [0, 1, 16, 0, 17, 0, 255] and want["bleaves"] == [3, 2, 6]
    if which == "shared position":
        assert want["cblock"][2] == 0 and want["coff"][2:4] == [16, 16] and want["braw"][1] == 16 + 17 and want["block_chunks"] == [8]
    assert tables(run(driver, "store", si)) == want


# ---- base_table ----


def model_base_table(vi, offsets):
    p = parse_version_index(vi)
    off = [NOWHERE] * len(p["chunk_sizes"])
    for a, at in enumerate(offsets):
        if at == SKIP or not int(p["sizes"][a]):
            continue
        for c in p["idx"][int(p["starts"][a]) : int(p["starts"][a]) + int(p["counts"][a])].tolist():
            if off[c] == NOWHERE:
                off[c] = at
            at += int(p["chunk_sizes"][c])
    sizes = p["chunk_sizes"].tolist()
    return dict(max_chunk=[max(sizes, default=0)], hash=p["chunk_hashes"].tolist(), size=sizes, off=off)


def dense(vi, skip):
    """-> (offsets, base_bytes): the resident assets one behind the other from byte 7 on, the others SKIP."""
    offsets, at = [], 7
    for a, size in enumerate(parse_version_index(vi)["sizes"].tolist()):
        offsets.append(SKIP if a in skip else at)
        at += 0 if a in skip else size
    return offsets, at


# chunks 3 and 4 lie in asset 1 alone; asset 3 is an empty file
SPLIT_ASSETS = [[0, 1, 2], [3, 4], [5, 6, 0], []]


@pytest.mark.parametrize("skip", [(1,), (0, 2)])
def test_base_table_of_the_sweep_version_with_every_second_asset_skipped(driver, skip):
    vi = sweep_version(HASHES)[0]
    offsets, base_bytes = dense(vi, skip)
    want = model_base_table(vi, offsets)
    assert NOWHERE not in want["off"]  # (every chunk of the sweep lies in every asset)
    assert tables(run(driver, "base", vi, offsets, base_bytes)) == want


def test_base_table_chunks_of_skipped_assets_are_nowhere_and_an_empty_asset_lies_anywhere(driver):
    vi = build_version_index(BLK3, 32768, ["a", "b", "c", "empty"], SPLIT_ASSETS, HASHES, LENGTHS)
    offsets, base_bytes = dense(vi, skip=(1,))
    offsets[3] = 2**63 + 5  # a zero-size resident asset: its offset is not looked at
    want = model_base_table(vi, offsets)
    assert [o == NOWHERE for o in want["off"]] == [False, False, False, True, True, False, False]
    assert tables(run(driver, "base", vi, offsets, base_bytes)) == want


@pytest.mark.parametrize("case", ["one byte past the base", "offset + size wraps 2^64"])
def test_base_table_refuses_a_window_that_leaves_the_base(driver, case):
    vi = sweep_version(HASHES)[0]
    offsets, base_bytes = dense(vi, skip=())
    assert tables(run(driver, "base", vi, offsets, base_bytes))["off"][0] == 7  # (the window that ends AT base_bytes is accepted)
    if case == "one byte past the base":
        base_bytes -= 1
    else:
        offsets[1] = 2**64 - 2  # (not SKIP; the asset has more than two bytes)
    assert run(driver, "base", vi, offsets, base_bytes) == [f"refused {errno.EINVAL} {LEAVES_BASE}"]


# ---- whole_asset_windows ----


def model_whole(vi, offsets):
    sizes = parse_version_index(vi)["sizes"].tolist()
    return [f"{a} 0 {size} {at if size else 0}" for a, (size, at) in enumerate(zip(sizes, offsets)) if at != SKIP]


def test_whole_asset_windows(driver):
    vi = sweep_version(HASHES)[0]
    offsets, _ = dense(vi, skip=())
    sizes = [sum(LENGTHS[c] for c in cs) for cs in SWEEP_ASSETS]
    assert run(driver, "whole", vi, offsets) == [f"{a} 0 {sizes[a]} {offsets[a]}" for a in range(3)] == model_whole(vi, offsets)
    assert run(driver, "whole", vi, [SKIP] * 3) == []
    # a directory and an empty file with nonsense offsets: windows of no bytes at offset 0
    vi = build_version_index(BLK3, 32768, ["dir/", "a", "empty", "b"], [[], [0, 1, 2], [], [3, 4]], HASHES[:5], LENGTHS[:5])
    offsets = [2**64 - 2, 64, 12345678901234567, SKIP]
    assert run(driver, "whole", vi, offsets) == ["0 0 0 0", f"1 0 {1 + 15 + 16} 64", "2 0 0 0"] == model_whole(vi, offsets)
