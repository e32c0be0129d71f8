"""CPU-only: the repack session's host arithmetic (longtail_amd/csrc/repack_plan.h over restore_parse.h) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program (tests/san/repack_plan_driver.cpp, its own
main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program -- nothing is preloaded.  Its answers are
checked line for line against a Python model of the layout: staging offsets, image offsets and their alignment, the tag-0 destinations
inside the images, the bounds, and the refusal of a block whose raw size leaves 32 bits.  The blobs lie at odd addresses and end where
their allocation ends."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.repack_util import own_tags
from tests.restore_util import BLK3, build_store_index

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "repack_plan_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
LZ4, ZTD3 = 0x6C7A3432, 0x7A746433
EINVAL, EBADF = 22, 9


def align8(x):
    return (x + 7) // 8 * 8


def bound(tag, raw):
    return raw + raw // 255 + 16 if tag == LZ4 else raw + raw // 256 + 64


def model(blocks, lens):
    """blocks: [(hash, tag, [chunk])] of a new index (its chunks in turn) -> the driver's lines."""
    raw = [sum(lens[c] for c in cs) for _, _, cs in blocks]
    stage, staged = [], 0
    for (_, tag, _), r in zip(blocks, raw):
        stage.append(staged if tag else -1)
        staged += r if tag else 0
    staging = align8(staged)
    lines, end, first = [], staging, 0
    for b, (_, tag, cs) in enumerate(blocks):
        hdr = 20 + 12 * len(cs) + (8 if tag else 0)
        cap = hdr + (bound(tag, raw[b]) if tag else raw[b])
        assert end % 8 == 0
        dest = stage[b] if tag else end + hdr
        lines.append(f"block {b} first {first} raw {raw[b]} tag {tag} stage {stage[b]} image {end} cap {cap} dest {dest}")
        end += align8(cap)
        first += len(cs)
    return lines + [f"staging {staging}", f"work {end}", f"moved {sum(raw)}"]


def new_index(counts_tags, lens_of):
    blocks, at = [], 0
    for k, (n, tag) in enumerate(counts_tags):
        blocks.append((0xAB000000 + k, tag, list(range(at, at + n))))
        at += n
    lens = [lens_of(c) for c in range(at)]
    hashes = np.arange(1000, 1000 + at, dtype=np.uint64)
    return blocks, lens, build_store_index(BLK3, blocks, hashes, lens)


CASES = {
    "every kind": ([(1, 0), (64, LZ4), (65, 0), (130, ZTD3), (3, LZ4), (2, 0)], lambda c: 1 + (c * 7) % 40),
    "tag 0 only": ([(5, 0), (1, 0), (9, 0)], lambda c: 1 + c % 3),
    "tagged only": ([(4, LZ4), (4, ZTD3)], lambda c: 33 + c),
    "large chunks": ([(2, LZ4), (3, 0)], lambda c: (1 << 30) - c),  # (the sums stay below 2^32, the offsets leave 32 bits)
    "nothing": ([], lambda c: 1),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("repack_plan")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "repack_plan_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


@pytest.mark.parametrize("case", list(CASES))
def test_the_layout_line_for_line_without_a_sanitizer_report(driver, case):
    exe, out = driver
    blocks, lens, blob = new_index(*CASES[case])
    # a store of five blocks with mixed tags; the kept index names the third and the first, under tags that are not theirs
    store_blocks = [(0x51 + k, tag, [2 * k, 2 * k + 1]) for k, tag in enumerate((0, LZ4, ZTD3, 0, LZ4))]
    sh, sl = np.arange(1, 11, dtype=np.uint64), list(range(1, 11))
    store = build_store_index(BLK3, store_blocks, sh, sl)
    kept = build_store_index(BLK3, [(store_blocks[2][0], 17, store_blocks[2][2]), (store_blocks[0][0], 9, store_blocks[0][2])], sh, sl)
    for name, data in (("new.bin", blob), ("store.bin", store), ("kept.bin", kept)):
        (out / name).write_bytes(data)
    run = subprocess.run([str(exe), str(out / "new.bin"), str(out / "store.bin"), str(out / "kept.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    lines = run.stdout.splitlines()
    want = model(blocks, lens)
    assert lines[: len(want)] == want
    assert lines[len(want)] == "kept 1 0 1 0 0"
    fixed = own_tags(kept, store)
    assert fixed != kept and lines[len(want) + 1] == "tags " + fixed.hex()
    assert lines[len(want) + 2] == f"refused {EINVAL} {EBADF} {EBADF}"
    assert lines[-1] == "ok"
