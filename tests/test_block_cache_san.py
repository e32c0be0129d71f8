"""CPU-only: the bookkeeping of the device cache of decoded blocks (longtail_amd/csrc/block_cache.h) under AddressSanitizer and
UndefinedBehaviorSanitizer.  The header has no line of HIP, so a small stand-alone program (tests/san/block_cache_driver.cpp, its own
main) includes it alone, is compiled with -fsanitize=address,undefined and run as a program -- nothing is preloaded.  It replays a
script this test writes: 5 000 seeded attach / reserve / commit / abort / unpin / clear operations over 4 slots and 12 keys, among them
reserve with everything pinned, commit of a key that already has an entry, attaches with mismatching digests, blocks larger than a
slot, and every operation on a slot that is in no state for it.  After every operation the driver prints the slots, the LRU order and
the counters; all of it must equal the Python model's (tests/block_cache_util.py), without a sanitizer report."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.block_cache_util import NO_SLOT, RESERVED, VISIBLE, CacheModel, table_digest

ROOT = Path(__file__).resolve().parent.parent
DRIVER = ROOT / "tests" / "san" / "block_cache_driver.cpp"
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SLOTS, SLOT_BYTES, KEYS = 4, 1000, 12  # (1000 rounds up to 1024)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    out = tmp_path_factory.mktemp("block_cache")
    probe = subprocess.run([cxx, *FLAGS, "-x", "c++", "-", "-o", str(out / "probe")], input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(out / "probe")]).returncode != 0:
        pytest.skip("the host compiler has no sanitizer runtime")
    exe = out / "block_cache_driver"
    build = subprocess.run([cxx, *FLAGS, str(DRIVER), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    return exe, out


def replay(driver, script, slots=SLOTS, slot_bytes=SLOT_BYTES):
    exe, out = driver
    (out / "script.txt").write_text("\n".join(script) + "\n")
    got = subprocess.run([str(exe), str(out / "script.txt"), str(slots), str(slot_bytes)], capture_output=True, text=True, timeout=300)
    assert got.returncode == 0, (got.stdout[-2000:], got.stderr[-4000:])
    assert "ERROR" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-4000:]
    lines = got.stdout.splitlines()
    assert lines[-1] == f"ok {len(script)}"
    return lines[:-1]


def key_of(k):
    return (0x626C6B33 if k % 4 else 0x626C6B32, 1000 + k // 2)  # keys that share a block hash under another identifier


def meta_of(k, variant=0):
    """What the StoreIndex says of key k; variant 1: another digest, 2: another raw size, 3: another chunk count."""
    raw = 1024 if k == 3 else 1025 if k == 7 else 10 + k  # key 3 fills a slot exactly, key 7 is one byte too large
    return (1 + k + (variant == 3), raw + (variant == 2), (0x1234567890ABCDEF * (k + 1) + (variant == 1)) % 2**64)


def scripted(seed, count):
    """-> (script lines, the model's line after each, how often each interesting case came up)."""
    rng = np.random.default_rng(seed)
    model = CacheModel(SLOTS, SLOT_BYTES)
    script, want = [], []
    seen = dict(reserve_all_pinned=0, commit_existing=0, commit_existing_pinned=0, mismatch=0, unverified=0, too_large=0, evicted_lru=0,
                clear_busy=0, clear_done=0, misuse=0, reuse_in_place=0)

    def emit(line, result):
        script.append(line)
        want.append(model.line(result))

    for _ in range(count):
        states = [s.state for s in model.slots]
        pinned = [i for i, s in enumerate(model.slots) if s.state == VISIBLE and s.pins]
        reserved = [i for i, s in enumerate(model.slots) if s.state == RESERVED]
        op = rng.choice(["attach", "attach", "reserve", "reserve", "commit", "abort", "unpin", "unpin", "clear", "misuse"],
                        p=[0.2, 0.1, 0.2, 0.1, 0.17, 0.04, 0.1, 0.05, 0.02, 0.02])
        k = int(rng.integers(0, KEYS))
        if op == "attach":
            variant = int(rng.choice([0, 0, 0, 1, 2, 3]))
            need = int(rng.integers(0, 2))
            i = model.lookup(key_of(k))
            if i != NO_SLOT and variant:
                seen["mismatch"] += 1
            if i != NO_SLOT and not variant and need and not model.slots[i].verified:
                seen["unverified"] += 1
            key, meta = key_of(k), meta_of(k, variant)
            emit(f"attach {key[0]} {key[1]} {meta[0]} {meta[1]} {meta[2]} {need}", model.attach(key, meta, bool(need)))
        elif op == "reserve":
            key, meta = key_of(k), meta_of(k, int(rng.choice([0, 0, 1])))
            mine = model.lookup(key)
            if meta[1] > model.slot_bytes:
                seen["too_large"] += 1
            elif mine != NO_SLOT:
                seen["reuse_in_place"] += not model.slots[mine].pins
            elif "F" not in states:
                if all(s.state == RESERVED or s.pins for s in model.slots):
                    seen["reserve_all_pinned"] += 1
                else:
                    seen["evicted_lru"] += 1
            emit(f"reserve {key[0]} {key[1]} {meta[0]} {meta[1]} {meta[2]}", model.reserve(key, meta))
        elif op == "commit" and reserved:
            i = int(rng.choice(reserved))
            other = model.lookup(model.slots[i].key)
            if other != NO_SLOT:
                seen["commit_existing"] += 1
                seen["commit_existing_pinned"] += bool(model.slots[other].pins)
            verified = int(rng.integers(0, 2))
            emit(f"commit {i} {verified}", model.commit(i, verified))
        elif op == "abort" and reserved:
            i, bad = int(rng.choice(reserved)), int(rng.integers(0, 2))
            emit(f"abort {i} {bad}", model.abort(i, bad))
        elif op == "unpin" and pinned:
            i = int(rng.choice(pinned))
            emit(f"unpin {i}", model.unpin(i))
        elif op == "clear":
            done = model.clear()
            seen["clear_done" if done else "clear_busy"] += 1
            emit("clear", done)
        else:  # an operation on a slot that is in no state for it, or on no slot at all: refused, nothing changes
            i = int(rng.integers(0, SLOTS + 2))
            what = str(rng.choice(["commit", "abort", "unpin"]))
            ok = i < SLOTS and ((what == "unpin" and i in pinned) or (what != "unpin" and i in reserved))
            if ok:
                continue
            seen["misuse"] += 1
            emit(f"{what} {i}" + ("" if what == "unpin" else " 1"), False)
    return script, want, seen


def test_five_thousand_operations_equal_the_model_without_a_sanitizer_report(driver):
    script, want, seen = scripted(seed=20, count=5600)
    script, want = script[:5000], want[:5000]
    assert len(script) == 5000
    assert all(v > 0 for v in seen.values()), seen
    got = replay(driver, script)
    for n, (g, w) in enumerate(zip(got, want)):
        assert g == w, (n, script[n], g, w)
    assert len(got) == len(want)


def test_the_digest_is_fnv1a_over_hashes_and_sizes(driver):
    tables = [([], []), ([0], [0]), ([2**64 - 1, 1, 0x0123456789ABCDEF], [2**32 - 1, 0, 77]), (list(range(100, 164)), list(range(64)))]
    script = [f"digest {len(h)} " + " ".join(f"{a} {b}" for a, b in zip(h, z)) for h, z in tables]
    got = replay(driver, script)
    assert got == [f"digest {table_digest(h, z)}" for h, z in tables]
    assert len({table_digest(h, z) for h, z in tables}) == len(tables)
    assert table_digest([1, 2], [3, 4]) != table_digest([2, 1], [3, 4]) != table_digest([1, 2], [4, 3])


def test_one_slot_and_a_block_that_fills_it_exactly(driver):
    model = CacheModel(1, 64)
    script, want = [], []
    for line, fn in [("reserve 1 5 1 64 9", lambda: model.reserve((1, 5), (1, 64, 9))), ("reserve 1 6 1 64 9", lambda: model.reserve((1, 6), (1, 64, 9))),
                     ("commit 0 1", lambda: model.commit(0, 1)), ("reserve 1 7 1 65 9", lambda: model.reserve((1, 7), (1, 65, 9))),
                     ("attach 1 5 1 64 9 1", lambda: model.attach((1, 5), (1, 64, 9), True)), ("reserve 1 6 1 64 9", lambda: model.reserve((1, 6), (1, 64, 9))),
                     ("clear", model.clear), ("unpin 0", lambda: model.unpin(0)), ("reserve 1 6 1 64 9", lambda: model.reserve((1, 6), (1, 64, 9))),
                     ("abort 0 1", lambda: model.abort(0, 1)), ("clear", model.clear)]:
        result = fn()
        script.append(line)
        want.append(model.line(result))
    assert replay(driver, script, slots=1, slot_bytes=1) == want
    assert (model.hits, model.inserted, model.evicted, model.bypassed, model.dropped) == (1, 1, 1, 3, 1)
