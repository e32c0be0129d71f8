"""CPU-only: the host side of a restore session's blocks call (longtail_amd/csrc/restore_call.h) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program (tests/san/restore_call_driver.cpp, its own
main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program -- nothing is preloaded.  The hash, offset
and size arrays of every call lie at ODD addresses that end where their allocation ends.  The state is six blocks: tags [0, LZ4, zstd,
0, 0x12345678, LZ4]; block 3 has no entries (not needed), block 5 is cache-fed, the others are needed.  Every line the program prints --
the refusal of a call and its reason, an accepted call's blocks, groups, counters and scratch sum, the pick from an archive window -- must
be the line of the Python model below, and a refused call must leave the state as it was (the program checks that itself)."""
import errno
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "restore_call_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
LZ4, ZSTD, ODD_TAG = 0x6C7A3432, 0x7A746433, 0x12345678
HASH = [0x1111111111111111 * (b + 1) for b in range(6)]
UNKNOWN = 0xDEADBEEFDEADBEEF
TAG = [0, LZ4, ZSTD, 0, ODD_TAG, LZ4]
CHUNKS = [1, 2, 3, 1, 1, 2]
RAW = [100, 200, 300, 64, 50, 129]
ENTRIES = [1, 2, 1, 0, 1, 1]
FED = [0, 0, 0, 0, 0, 1]
SCRATCH, OUT, OTHER = 0x10000, 0x20000, 0x30000  # pointers: numbers that are never followed


def round64(x):
    return (x + 63) // 64 * 64


class Model:
    """What restore_call.h is to compute, stated once more: about forty lines."""

    def __init__(self, entries=ENTRIES):
        self.entries, self.delivered, self.counters = list(entries), set(), [0, 0, 0]
        self.needed_count = sum(self.needed(b) for b in range(6))

    def needed(self, b):
        return self.entries[b] > 0 and not FED[b]

    def slot(self, b):
        return round64(RAW[b]) if self.needed(b) and TAG[b] else 0

    def bound(self, hashes):
        return sum(self.slot(HASH.index(h)) for h in hashes if h in HASH)

    def call(self, hashes, offsets, sizes, any_position=0, scratch=SCRATCH, scratch_bytes=1 << 20, out=OUT, in_place=0):
        def refused(code, why):
            return f"refused {code} {why}"

        blocks, total = [], 0
        for h, off in zip(hashes, offsets):
            if h not in HASH:
                return refused(errno.ENOENT, "a block hash the store index does not hold")
            b = HASH.index(h)
            if b in self.delivered or b in blocks:
                return refused(errno.EEXIST, "a block was delivered before, or twice in this call")
            blocks.append(b)
            if not any_position and off % 8:
                return refused(errno.EINVAL, "image offsets must be 8-byte aligned")
            if self.needed(b) and TAG[b] not in (0, LZ4, ZSTD):
                return refused(errno.ENOTSUP, "a needed block's tag names no codec of this library")
            total += self.slot(b)
        any_needed = any(self.needed(b) for b in blocks)
        if total > scratch_bytes:
            return refused(errno.ENOMEM, "scratch below lthip_restore_scratch_bound")
        if (total and not scratch) or (any_needed and not out):
            return refused(errno.EINVAL, "null scratch or output")
        if any_needed and in_place and out != in_place:
            return refused(errno.EINVAL, "the base was carried in place: the output is that buffer")
        groups = [[], [], []]
        for i, (b, size) in enumerate(zip(blocks, sizes)):
            self.delivered.add(b)
            self.counters[0 if self.needed(b) else 2] += 1
            self.counters[1] += 1
            if self.needed(b):
                payload = size > 20 + 12 * CHUNKS[b] + 8
                groups[0 if not TAG[b] or not payload else 1 if TAG[b] == LZ4 else 2].append(i)
        text = lambda v: ",".join(str(x) for x in v)
        return (f"ok blocks={text(blocks)} scratch={total} any={int(any_needed)} groups={'|'.join(text(g) for g in groups)} "
                f"counters={self.needed_count},{text(self.counters)} bound={self.bound(hashes)}")

    def pick(self, archive, body, first, nbytes):
        end, nxt, blocks, offsets, sizes = min(first + nbytes, 2**64 - 1), body, [], [], []
        for h, off, size in archive:
            b = HASH.index(h) if h in HASH else None
            if b is None or not self.needed(b) or b in self.delivered or b in blocks:
                continue
            if off < first or off + size > end:
                nxt = min(nxt, off)
            else:
                blocks.append(b), offsets.append(off - first), sizes.append(size)
        text = lambda v: ",".join(str(x) for x in v)
        return f"pick blocks={text(blocks)} offsets={text(offsets)} sizes={text(sizes)} scratch={sum(self.slot(b) for b in blocks)} next={nxt}"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("restore_call")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "restore_call_driver"
    build = subprocess.run([cxx, *FLAGS, "-Wno-unused-function", str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


class Script:
    """The steps of one run of the program and, beside each, the line the model expects."""

    def __init__(self, out, name):
        self.out, self.name, self.lines, self.expected, self.files = out, name, [], [], 0
        for b in range(6):
            self.lines.append(f"block {HASH[b]} {TAG[b]} {CHUNKS[b]} {RAW[b]} {ENTRIES[b]} {FED[b]}")
        self.reset()

    def reset(self, entries=ENTRIES):
        self.lines += [f"entries {b} {n}" for b, n in enumerate(entries)] + ["reset"]
        self.model = Model(entries)

    def call(self, blocks, offsets=None, sizes=None, by_index=False, **kw):
        """blocks: indices, or a hash the state does not hold"""
        hashes = [HASH[b] if b < 6 else b for b in blocks]
        offsets = [64 * i for i in range(len(blocks))] if offsets is None else offsets
        sizes = [1000] * len(blocks) if sizes is None else sizes
        path = self.out / f"{self.name}_{self.files}.bin"
        self.files += 1
        path.write_bytes(np.array(hashes, np.uint64).tobytes() + np.array(offsets, np.uint64).tobytes() + np.array(sizes, np.uint32).tobytes())
        a = dict(any_position=0, scratch=SCRATCH, scratch_bytes=1 << 20, out=OUT, in_place=0)
        a.update(kw)
        self.lines.append(f"{'calli' if by_index else 'call'} {path} {len(blocks)} {a['any_position']} {a['scratch']} {a['scratch_bytes']} "
                          f"{a['out']} {a['in_place']}")
        self.expected.append(self.model.call(hashes, offsets, sizes, **a))
        return self.expected[-1]

    def run(self, exe):
        path = self.out / f"{self.name}.txt"
        path.write_text("\n".join(self.lines) + "\n")
        run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
        assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
        assert run.stdout.splitlines() == self.expected + ["done"]


def test_refusals_are_the_first_position_that_refuses_and_change_nothing(driver):
    exe, out = driver
    s = Script(out, "refusals")
    code = lambda line: int(line.split()[1]) if line.startswith("refused") else 0
    # 1. an unknown hash; the call's good blocks are delivered afterwards (as after every refusal below)
    assert code(s.call([0, UNKNOWN])) == errno.ENOENT
    # 2. twice in the call
    assert code(s.call([1, 2, 1])) == errno.EEXIST
    assert code(s.call([0])) == 0
    # 3. delivered by an earlier accepted call
    assert code(s.call([1, 0])) == errno.EEXIST
    # 4. a misaligned offset before an unknown hash, and the two swapped
    assert code(s.call([1, UNKNOWN], offsets=[4, 8])) == errno.EINVAL
    assert code(s.call([UNKNOWN, 1], offsets=[8, 4])) == errno.ENOENT
    # 5. the same misaligned call at any position: the unknown hash is what is left to refuse; without it, accepted
    assert code(s.call([1, UNKNOWN], offsets=[4, 8], any_position=1)) == errno.ENOENT
    assert code(s.call([1], offsets=[4])) == errno.EINVAL
    assert code(s.call([1], offsets=[4], any_position=1)) == 0
    # 6. a needed block whose tag names no codec; the same tag on a block that is not needed
    assert code(s.call([2, 4])) == errno.ENOTSUP
    assert code(s.call([2])) == 0
    s.reset([1, 2, 1, 0, 0, 1])
    assert code(s.call([2, 4])) == 0
    s.reset()
    # 7. scratch one below the sum, then the sum
    total = round64(RAW[1]) + round64(RAW[2])
    assert code(s.call([0, 1, 2], scratch_bytes=total - 1)) == errno.ENOMEM
    assert code(s.call([0, 1, 2], scratch_bytes=total)) == 0
    s.reset()
    # 8. null scratch with a tagged needed block, null output with a needed block, only block 3 with null output and scratch
    assert code(s.call([0, 1], scratch=0)) == errno.EINVAL
    assert code(s.call([0], scratch=0, out=0)) == errno.EINVAL
    assert code(s.call([0], scratch=0, scratch_bytes=0)) == 0
    assert code(s.call([3, 5], scratch=0, scratch_bytes=0, out=0)) == 0
    # 9. an in-place buffer that is not the output; a call without a needed block does not care
    assert code(s.call([1], in_place=OTHER)) == errno.EINVAL
    assert code(s.call([1], in_place=OUT)) == 0
    s.reset()
    assert code(s.call([3], in_place=OTHER)) == 0
    s.run(exe)


@pytest.mark.parametrize("by_index", [False, True])
def test_accepted_calls_give_groups_counters_and_the_scratch_sum_of_the_bound(driver, by_index):
    exe, out = driver
    s = Script(out, f"accepted{int(by_index)}")
    hdr = lambda b: 20 + 12 * CHUNKS[b] + 8
    # every deliverable block (4 is needed and names no codec) in two orders; an LZ4 image no longer than its header is not decoded
    line = s.call([0, 1, 2, 3, 5], sizes=[1000, hdr(1), hdr(2) + 1, 500, 700], by_index=by_index)
    assert "groups=0,1||2 " in line and f"scratch={round64(200) + round64(300)} " in line and line.endswith(f"bound={round64(200) + round64(300)}")
    assert "counters=4,3,5,2" in line
    s.reset()
    line = s.call([5, 2, 1, 3, 0], sizes=[700, hdr(2) + 1, hdr(1) + 1, 500, 20 + 12], by_index=by_index)
    assert "groups=4|2|1 " in line and "counters=4,3,5,2" in line
    if not by_index:  # the bound counts nothing for an unknown hash, an unneeded block and a fed one
        s.reset()
        assert s.call([UNKNOWN]).startswith("refused")
        assert s.call([3, 5, 1], scratch_bytes=round64(200)).endswith(f"bound={round64(200)}")
    s.run(exe)


def test_a_call_counter_that_wraps_clears_the_stamps(driver):
    exe, out = driver
    s = Script(out, "stamps")
    for wrapping in ([1, 2, 1], [1, 2]):
        s.reset()
        assert s.call([1, 2, 1]).startswith("refused 17")  # call number 1 stamps blocks 1 and 2 with 1
        s.lines.append(f"stamp {0xFFFFFFFF}")
        # the counter wraps to call number 1 again: were the table not cleared, the stale stamps would have [1, 2] refused
        assert s.call(wrapping).startswith("ok" if wrapping == [1, 2] else "refused 17")
        # ... and the call after it
        assert s.call([0, 3, 0]).startswith("refused 17")
        assert s.call([0, 3]).startswith("ok")
    s.run(exe)


def test_the_pick_from_an_archive_window(driver):
    exe, out = driver
    s = Script(out, "pick")
    # eight entries: block 1 twice, a hash the session does not hold, block 3 (not needed), block 5 (fed), block 0 (delivered below)
    archive = [(HASH[1], 0, 100), (HASH[0], 100, 50), (HASH[1], 150, 100), (UNKNOWN, 250, 10), (HASH[3], 260, 40), (HASH[5], 300, 60),
               (HASH[2], 360, 80), (HASH[4], 440, 30)]
    body = 470
    assert s.call([0]).startswith("ok")
    s.lines += [f"archive {body} {len(archive)}"] + [f"{h} {o} {z}" for h, o, z in archive]
    windows = [(0, body), (0, 400), (50, 350), (100, 0), (100, 2**64 - 50), (2**64 - 10, 100), (0, 2**64 - 1)]
    for first, nbytes in windows:
        s.lines.append(f"pick {first} {nbytes}")
        s.expected.append(s.model.pick(archive, body, first, nbytes))
    assert s.expected[1] == f"pick blocks=1,2,4 offsets=0,360,440 sizes=100,80,30 scratch={256 + 320 + 64} next=470"
    assert s.expected[2].endswith("next=360") and "blocks=1 " in s.expected[2]  # the window cuts block 2 in the middle
    assert s.expected[3].startswith("pick blocks=1 offsets=100 ") and s.expected[3].endswith("next=0")  # block 1's second listing
    assert s.expected[4] == "pick blocks= offsets= sizes= scratch=0 next=0"
    assert s.expected[5].startswith("pick blocks=1,2,4 offsets=50,260,340 ")  # first + bytes wraps: the window runs to the end
    s.run(exe)
