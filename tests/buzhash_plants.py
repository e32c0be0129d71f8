"""Bytes built so that the Buzhash-48 chunker cuts where a test chooses (CPU, numpy only).

H(p), the hash that decides whether a chunk may end at p, is a pure function of the 48 bytes before p, and it is GF(2)-linear in a choice
between two byte values per position: with two random 48-byte strings b0, b1 the 48 difference vectors rotl(T[b0[i]] ^ T[b1[i]], 47 - i)
almost always span all 32 bits, and Gaussian elimination picks the positions that take b1's byte so that the window hashes to any wanted
value (window_for).  A part is zero bytes -- the hash of 48 zero bytes is 0x9E489E48, a candidate for no discriminator used here -- with
such windows planted in it (planted_part); a window is drawn again until the positions around it that see a part of it are no candidates
by chance, and the finished part is held against the oracle's own candidate scan: its candidate set is the planted one and nothing else.

The cases (sweep, sparse_sweep, div_edges, select, dense, guess) put cuts in every (lane, step) class of a wave-tile, on the edges of the
cut test's arithmetic, in the arrangements of k_select_cuts' search, several to a tile, and where the walking scan's prefetch guesses
wrong.  tests/test_buzhash_plants_cases.py proves on the CPU that they are what they claim, tests/test_gpu_buzhash_plants.py runs them
through the scans.  walk_trace follows the walking scan's path over a part, so that the cases can show which of its branches they take;
model_lengths is a small numpy model of the tile scan's candidates and of the selection, with switches that break one
rule each: the CPU test shows that every such defect changes an answer on some case (no kernel is ever run broken)."""
from __future__ import annotations

import functools
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

from tests._libs import oracle

ROOT = Path(__file__).resolve().parent.parent
WINDOW = 48
M32 = 0xFFFFFFFF
WTILE = 4096  # a wave-tile: 64 lanes x 64 steps
ZERO_HASH = 0x9E489E48  # H of 48 zero bytes
TABLE = np.array([int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{8})u", (ROOT / "longtail_amd/csrc/buzhash_table.inc").read_text())],
                 dtype=np.uint32)
assert len(TABLE) == 256
_T = [int(x) for x in TABLE]

# averages whose discriminator is a power of two (the reference's formula, hpcdcchunker.c:126-129)
POW2_AVERAGES = {86: 64, 171: 128, 342: 256, 683: 512, 1365: 1024, 2728: 2048, 5455: 4096, 10903: 8192, 21779: 16384, 43456: 32768,
                 86509: 65536}


def reference_discriminator(avg: int) -> int:
    return int(float(avg) / (-1.42888852e-7 * float(avg) + 1.33237515))


def disc(avg: int) -> int:
    return int(oracle().dll.lto_hpcdc_discriminator(avg))


def is_pow2(d: int) -> bool:
    return d & (d - 1) == 0


def _rotl(x: int, r: int) -> int:
    r &= 31
    return ((x << r) | (x >> (32 - r))) & M32 if r else x


def _rotl_np(x: np.ndarray, r: int) -> np.ndarray:
    r &= 31
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r)) if r else x


def buzhash(window) -> int:
    """H of a 48-byte window (window[47] is the newest byte)."""
    h = 0
    for i, b in enumerate(window):
        h ^= _rotl(_T[int(b)], 47 - i)
    return h


def hashes(a: np.ndarray) -> np.ndarray:
    """H(p) for p = 48 .. len(a): element p - 48."""
    u = TABLE[a]
    n = len(a)
    h = np.zeros(n - 47, np.uint32)
    for j in range(WINDOW):
        h ^= _rotl_np(u[47 - j : n - j], j)
    return h


def window_for(target: int, rng) -> np.ndarray:
    """48 bytes whose hash is exactly `target`."""
    while True:
        b0, b1 = rng.integers(0, 256, (2, WINDOW), dtype=np.uint8)
        basis = {}  # highest set bit -> (vector, the positions that make it)
        for i in range(WINDOW):
            v, m = _rotl(_T[int(b0[i])] ^ _T[int(b1[i])], 47 - i), 1 << i
            while v:
                top = v.bit_length() - 1
                if top not in basis:
                    basis[top] = (v, m)
                    break
                v, m = v ^ basis[top][0], m ^ basis[top][1]
        v, m = buzhash(b0) ^ target, 0
        while v and v.bit_length() - 1 in basis:
            bv, bm = basis[v.bit_length() - 1]
            v, m = v ^ bv, m ^ bm
        if v:
            continue  # (the difference vectors do not reach it: other strings)
        take = np.array([(m >> i) & 1 for i in range(WINDOW)], bool)
        return np.where(take, b1, b0)


def is_candidate(h, d: int):
    return h % d == d - 1


def candidate_hash(d: int, rng) -> int:
    return int(rng.integers(0, (1 << 32) // d)) * d + d - 1


def candidates(a: np.ndarray, d: int) -> np.ndarray:
    """The oracle's candidate set of a whole part: every p in [48, len] with H(p) % d == d - 1."""
    bm = np.zeros(len(a) // 8 + 2, np.uint8)
    if len(a):
        oracle().dll.lto_hpcdc_candidates(a.ctypes.data, len(a), d, bm.ctypes.data)
    return np.flatnonzero(np.unpackbits(bm, bitorder="little"))


class BuilderError(AssertionError):
    pass


@functools.lru_cache(maxsize=None)
def _clean_windows(d: int, target):
    """A handful of windows for (d, hash or None = any candidate) that are, planted in zeros, alone in their neighbourhood: the window's
    bytes do not depend on where it is put, so they serve every isolated plant of every part."""
    rng = np.random.default_rng([d, 0 if target is None else target + 1])
    out = []
    while len(out) < 4:
        w = window_for(candidate_hash(d, rng) if target is None else target, rng)
        buf = np.zeros(95 + WINDOW + 47, np.uint8)
        buf[95:143] = w
        hit = np.flatnonzero(is_candidate(hashes(buf), d)) + WINDOW
        if hit.tolist() == ([143] if is_candidate(buzhash(w), d) else []):
            out.append(w)
    return out


def _tail_fills(a, lo, p, d, target, rng):
    """The window that ends at p shares its bytes below `lo` with a plant before it: fills of [lo, p) that give the wanted hash."""
    n = p - lo
    fixed = 0
    for i in range(p - WINDOW, lo):
        fixed ^= _rotl(_T[int(a[i])], p - 1 - i)
    fills = np.arange(256, dtype=np.uint8)[:, None] if n == 1 else rng.integers(0, 256, (4096, n), dtype=np.uint8)
    h = np.full(len(fills), fixed, np.uint32)
    for c in range(n):
        h ^= _rotl_np(TABLE[fills[:, c]], p - 1 - (lo + c))
    return fills[(h == target) if target is not None else is_candidate(h, d)]


def planted_part(size: int, cuts, d: int, decoys=(), seed: int = 0) -> np.ndarray:
    """`size` zero bytes with a window ending at each position of `cuts` (a position p, or (p, hash) for a chosen candidate hash), so that
    p is a candidate for d, and at each (p, hash) of `decoys` a window with that non-candidate hash.  The oracle's candidate set over the
    whole part equals `cuts` and nothing else, or the builder fails."""
    assert not is_candidate(ZERO_HASH, d), d
    plants = []
    for c in cuts:
        p, h = c if isinstance(c, tuple) else (c, None)
        assert h is None or is_candidate(h, d), (p, h, d)
        plants.append((int(p), h, True))
    for p, h in decoys:
        assert not is_candidate(h, d), (p, h, d)
        plants.append((int(p), int(h), False))
    plants.sort()
    want = {p for p, _, cut in plants if cut}
    assert len({p for p, _, _ in plants}) == len(plants) and all(WINDOW <= p <= size for p, _, _ in plants)
    rng = np.random.default_rng([size, d, seed, len(plants)])
    a = np.zeros(size, np.uint8)
    lows = [0] * len(plants)  # where plant i's own bytes start
    again = set()  # plants drawn again for the sake of the one behind them: fresh windows, not the shared ones
    i = tries = 0
    while i < len(plants):
        tries += 1
        if tries > 20000:
            raise BuilderError(f"no part for d={d} size={size} plants={plants[:4]}...")
        p, target, cut = plants[i]
        end_before = plants[i - 1][0] if i else 0
        lo = max(p - WINDOW, end_before)
        lows[i] = lo
        isolated = p - 95 >= end_before and (i + 1 == len(plants) or plants[i + 1][0] - 95 >= p)
        if isolated and i not in again:
            pool = _clean_windows(d, target)
            a[lo:p] = pool[(i + seed) % len(pool)]
            i += 1
            continue
        if lo == p - WINDOW:
            a[lo:p] = window_for(candidate_hash(d, rng) if target is None else target, rng)
        else:
            fills = _tail_fills(a, lo, p, d, target, rng)
            if len(fills) == 0:  # the plant before it leaves no fill: draw that one again
                a[lows[i - 1] : p] = 0
                i -= 1
                again.add(i)
                continue
            a[lo:p] = fills[int(rng.integers(0, len(fills)))]
        # every position that sees a byte of this plant: a candidate only where one is planted (later plants are checked when they are made)
        x0, x1 = max(lo + 1, WINDOW), min(p + 47, size)
        h = hashes(a[x0 - WINDOW : x1])
        hit = set((np.flatnonzero(is_candidate(h, d)) + x0).tolist())
        if {x for x in hit if x <= p} != {x for x in want if x0 <= x <= p} or any(x not in want for x in hit):
            a[lo:p] = 0
            continue
        i += 1
    got = candidates(a, d)
    if got.tolist() != sorted(want):
        raise BuilderError(f"d={d} size={size}: candidates {got[:8]} of {len(got)}, planted {sorted(want)[:8]} of {len(want)}")
    for p, target, _ in plants:
        if target is not None and buzhash(a[p - WINDOW : p]) != target:
            raise BuilderError(f"d={d}: the window at {p} does not hash to {target:#x}")
    return a


def place(parts):
    """Part offsets in one buffer that cycle through the four 16-byte phases modulo 64 -> (offsets, total bytes)."""
    offs, pos = [], 0
    for i, p in enumerate(parts):
        pos += (16 * (i % 4) - pos) % 64
        offs.append(pos)
        pos += len(p)
    return offs, max(pos, 16)


def jump(q: int) -> int:
    """The walking scan's tile for a chunk whose first legal candidate is q (the comment above walk_body in k_buzhash.hip): the tile whose
    data starts at or below q, on a multiple of 16, with the 64 bytes in front of it as the halo row."""
    return ((q - 64) & ~15) + 64 if q >= 64 else 0


def walk_trace(lens, size: int, mn: int, mx: int, hashing: bool = True):
    """The path of the walking scan (walk_body in k_buzhash.hip, the form that guesses) over one part whose chunks are `lens`, for a wave
    that comes to it with an empty pending list: how many tiles it hashes, how often a chunk's first candidate lies in the tile already
    hashed (same_tile), how often the full pending list sends it to that tile again behind a round (rehash; hashing only), and what
    becomes of its prefetch guesses: used for the next 4 KiB (used_next) or for the jump behind a chunk that ends at `end` (used_jump),
    aimed elsewhere than the walk goes (wrong), or still in flight at the part's end (wasted)."""
    t = dict(tiles=0, same_tile=0, rehash=0, used_next=0, used_jump=0, wrong=0, wasted=0)
    s = i = pl = 0
    inflight = None  # (tile, kind) of the guess on its way
    tb = end = qlo = qhi = 0

    def classify():
        nonlocal end, qlo, qhi
        left = size - s
        n = left if left <= mn else min(left, mx)
        if not (left > mn and n > mn):
            return n
        end, qlo, qhi = n, s + mn, s + n - 1
        return None

    def emit(n):
        nonlocal s, i, pl
        assert n == lens[i], (i, n, lens[i])
        s, i, pl = s + n, i + 1, pl + max(1, (n + 1023) // 1024)

    scanning = False
    while True:
        if hashing and pl >= 64:
            pl -= 64
            continue
        if not scanning:
            if s >= size:
                t["wasted"] += inflight is not None
                return t
            n = classify()
            if n is not None:
                emit(n)
                continue
            tb, scanning = jump(qlo), True
        if inflight is not None:
            t["used_" + inflight[1] if inflight[0] == tb else "wrong"] += 1
        inflight = (tb + WTILE, "next")
        if qhi - tb < WTILE:  # the chunk ends in this tile at the latest: the guess is the jump behind it
            s2 = s + end
            inflight = (jump(s2 + mn), "jump") if size - s2 > mn and mx > mn else None
        t["tiles"] += 1
        while True:  # the chunks that end in this tile
            if s + lens[i] - 1 >= tb + WTILE:
                tb += WTILE
                break
            emit(lens[i])
            if s >= size or classify() is not None:
                scanning = False
                break
            if qlo - tb < WTILE and not (hashing and pl >= 64):
                t["same_tile"] += 1
                continue
            t["rehash"] += qlo - tb < WTILE
            tb = jump(qlo)
            break


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
Group = namedtuple("Group", "cfg parts labels")  # parts cut with the parameters cfg = (min, avg, max); labels[i] says what part i is
Case = namedtuple("Case", "name groups")

SWEEP_CFGS = [(512, 700, 8192), (512, 683, 8192)]  # d = 525, and the power of two 512
HEADLINE_CFGS = [(8192, 32768, 131072), (8192, 21779, 131072)]  # d = 24680 ... and 16384
SPARSE_LANES = (0, 1, 2, 31, 32, 62, 63)
SPARSE_STEPS = (0, 1, 15, 16, 17, 30, 31, 32, 46, 47, 48, 62, 63)


def _sweep_group(cfg, lengths):
    """One part per first cut length L; a second plant behind it at a distance that varies with L (the second chunk starts at L: every
    residue modulo 16, so its tile takes every alignment), then a tail of at most min bytes."""
    mn, av, mx = cfg
    d = disc(av)
    parts, labels = [], []
    for L in lengths:
        dist = mn + 1 + (L * 37) % 1021
        tail = 17 + L % min(mn, 400)
        parts.append(planted_part(L + dist + tail, [L, L + dist], d, seed=L))
        labels.append((L, dist))
    return Group(cfg, parts, labels)


@functools.lru_cache(maxsize=None)
def sweep():
    return Case("sweep", [_sweep_group(cfg, range(cfg[0] + 1, cfg[0] + 4161)) for cfg in SWEEP_CFGS])


def sparse_lengths(mn):
    """Cut lengths whose candidate bit q = L - 1 is base + 64 lane + step: from min on, across a 4 KiB and across a 16 KiB boundary."""
    out = []
    for base in (mn, mn + 2048, 16384 - 2048):
        out += [base + 64 * lane + step + 1 for lane in SPARSE_LANES for step in SPARSE_STEPS]
    return out


@functools.lru_cache(maxsize=None)
def sparse_sweep():
    return Case("sparse_sweep", [_sweep_group(cfg, sparse_lengths(cfg[0])) for cfg in HEADLINE_CFGS])


DIV_EDGE_CFGS = {24680: (256, 32768, 32768), 96: (64, 128, 4096), 75: (48, 100, 4096), 49535: (256, 65536, 65536), 64: (64, 86, 4096),
                 16384: (256, 21779, 32768)}


def div_edge_hashes(d: int):
    """-> (cuts, decoys): {label: hash}."""
    k2 = (d & -d).bit_length() - 1
    dodd = d >> k2
    cuts = {"H+1 = d": d - 1, "H+1 = the largest multiple of d": d * (M32 // d) - 1}
    decoys = {"H = 0": 0, "H = d-2": d - 2}
    if is_pow2(d):
        cuts["H = 0xFFFFFFFF"] = M32
        decoys["low bits all ones but bit 0"] = M32 ^ 1
        decoys["low bits all ones but the top one"] = 0x5A5A0000 | ((d - 1) ^ (d >> 1))
    else:
        decoys["H = 0xFFFFFFFF"] = M32
        if k2:
            m = M32 // dodd
            decoys["H+1 = the odd part of d"] = dodd - 1
            decoys["H+1 = a large odd multiple of the odd part"] = dodd * (m if m & 1 else m - 1) - 1
    return cuts, decoys


@functools.lru_cache(maxsize=None)
def div_edges():
    """Per d: for every planted cut a part with all the decoys in front of it (the chunk ends at the cut, at no decoy), and a part of
    decoys alone (the chunk runs to the part's end)."""
    groups = []
    for d, cfg in DIV_EDGE_CFGS.items():
        mn, av, mx = cfg
        assert disc(av) == d
        cuts, decoys = div_edge_hashes(d)
        parts, labels = [], []
        for n, (label, h) in enumerate(cuts.items()):
            at = [(mn + 60 + 150 * i + 13 * n, dh) for i, dh in enumerate(decoys.values())]
            p = mn + 60 + 150 * len(at) + 29 * n
            parts.append(planted_part(p + mn // 2 + n, [(p, h)], d, decoys=at, seed=n))
            labels.append((label, p, h, at))
        at = [(mn + 77 + 131 * i, dh) for i, dh in enumerate(decoys.values())]
        parts.append(planted_part(mn + 77 + 131 * len(at) + 5, [], d, decoys=at))
        labels.append(("decoys alone", None, None, at))
        groups.append(Group(cfg, parts, labels))
    return Case("div_edges", groups)


SELECT_CFGS = SWEEP_CFGS
SELECT_FAR_CFGS = [(8192, 65536, 524288), (8192, 21779, 524288)]  # a search over more than 64 level-1 words (256 KiB)


def _select_group(cfg, far):
    """Every part: a first chunk that ends at a planted cut s, chosen so that the second chunk's first legal candidate bit qlo = s + min
    sits where the arrangement needs it; label = (name, s)."""
    mn, av, mx = cfg
    d = disc(av)
    parts, labels = [], []

    def add(name, s, cand, size):
        parts.append(planted_part(size, ([s] if s else []) + [s + c for c in cand], d, seed=len(parts)))
        labels.append((name, s))

    def start(bit, run):  # s > min with qlo = s + min on bit `bit` of run `run` (modulo 64) of its level-1 word
        s = (run * 64 + bit - mn) % WTILE
        while s <= mn:
            s += WTILE
        return s

    if far:
        s = start(20, 10)
        add("decoy at min, cut more than 256 KiB behind", s, [mn, mn + 1 + 262144 + 2 * WTILE + 33], s + mn + 262144 + 3 * WTILE)
        return Group(cfg, parts, labels)
    s = start(20, 10)
    add("decoy at min, cut at min+1 in the same run", s, [mn, mn + 1], s + mn + 300)
    add("decoy at min, cut in a later run of the same word", s, [mn, mn + 1 + 5 * 64 + 7], s + mn + 700)
    add("decoy at min, cut in a later word", s, [mn, mn + 1 + WTILE + 100], s + mn + WTILE + 300)
    s = start(3, 40)
    add("two candidates in one run", s, [mn + 1, mn + 1 + 55], s + mn + 200)
    for bit in (30, 63):  # qhi = s + max - 1 on bit 30 (max+1 shares its run) and on bit 63 (max+1 opens the next run)
        s = start((bit + 1 - (mx - mn)) % 64, 7)
        add(f"candidate at max, qhi on bit {bit}", s, [mx], s + mx + mn + 9)
        add(f"candidate at max+1, qhi on bit {bit}", s, [mx + 1], s + mx + mn + 9)
        add(f"candidate at size, qhi on bit {bit}", s, [mx - 64], s + mx - 64)
    for bit, run in ((0, 0), (63, 0), (0, 63), (63, 63)):  # the first chunk's own cut, on the corners of the two bitmap levels
        q = WTILE + 64 * run + bit
        add(f"cut on bit {bit} of run {run}", 0, [q + 1], q + 1 + mn // 2)
    return Group(cfg, parts, labels)


@functools.lru_cache(maxsize=None)
def select():
    return Case("select", [_select_group(c, False) for c in SELECT_CFGS] + [_select_group(c, True) for c in SELECT_FAR_CFGS])


DENSE_CFGS = [(64, 128, 4096), (64, 86, 300)]  # d = 96 and the power of two 64


@functools.lru_cache(maxsize=None)
def dense():
    """Plants every 65 to 200 bytes, 150 chunks per part: several cuts in every tile, and more than 64 chunks pending in one wave."""
    groups = []
    for cfg in DENSE_CFGS:
        d = disc(cfg[1])
        parts, labels = [], []
        for k in range(4):
            gaps = [65 + (i * 37 + k * 11 + (i * i) % 7) % 136 for i in range(150)]
            cuts = np.cumsum(gaps).tolist()
            parts.append(planted_part(cuts[-1] + 10 + k, cuts, d, seed=k))
            labels.append(gaps)
        groups.append(Group(cfg, parts, labels))
    return Case("dense", groups)


@functools.lru_cache(maxsize=None)
def guess():
    """Cuts that make the walking scan's prefetch wrong (it aims at the next 4 KiB, or at the jump target behind a chunk that ends at
    max): a cut with a tail of at most min bytes behind it (the next chunk needs no scan), and a cut followed by a chunk that ends at max."""
    groups = []
    for cfg in HEADLINE_CFGS:
        mn, av, mx = cfg
        d = disc(av)
        parts, labels = [], []
        for n, (L, tail) in enumerate([(mn + 1001, 1), (mn + 1001, mn), (mn + 5000, 77), (mn + 1, mn - 1), (mn + WTILE, 48)]):
            parts.append(planted_part(L + tail, [L], d, seed=n))
            labels.append(("tail", L, tail))
        for n, (L, k) in enumerate([(mn + 1001, 701), (mn + 4097, 1), (mn + 64, 4100)]):
            third = L + mx + mn + k  # [cut at L][a chunk of max bytes][cut][a tail that reaches into the next tile]
            parts.append(planted_part(third + 5000 + n, [L, third], d, seed=10 + n))
            labels.append(("max", L, k))
        parts.append(planted_part(mx + mn, [], d))  # a chunk of max bytes, then a tail of exactly min: the guess is not aimed
        labels.append(("max then tail", mx, mn))
        groups.append(Group(cfg, parts, labels))
    return Case("guess", groups)


FROM_BUFFER_CFGS = [(512, 683, 8192), (8192, 21779, 131072), (64, 86, 300)]  # power-of-two discriminators: 512, 16384, 64


@functools.lru_cache(maxsize=None)
def from_buffer_plants():
    """For lthip_chunk_from_buffer: zero buffers with one window that ends k >= 48 bytes behind min -- behind the 47 lengths for which the
    reference's window still holds the buffer's first bytes -- drawn again until the oracle's NextChunkFromBuffer cuts there.
    -> [(cfg, buffer, the cut)]"""
    o = oracle().dll
    out = []
    for cfg in FROM_BUFFER_CFGS:
        mn, av, mx = cfg
        d = disc(av)
        rng = np.random.default_rng([d, mn])
        for k in (48, 49, 111):
            p = mn + k
            for _ in range(2000):
                a = np.zeros(p + 150, np.uint8)
                a[p - WINDOW : p] = window_for(candidate_hash(d, rng), rng)
                if int(o.lto_hpcdc_next_from_buffer(a.ctypes.data, len(a), mn, av, mx)) == p:
                    break
            else:
                raise BuilderError(f"no buffer for {cfg} that cuts at {p}")
            out.append((cfg, a, p))
    return out


CASES = {"sweep": sweep, "sparse_sweep": sparse_sweep, "div_edges": div_edges, "select": select, "dense": dense, "guess": guess}


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """The oracle's chunks of every part of a case, computed once: per group a list of (offsets, lengths, hashes), lengths from
    lto_hpcdc_chunk_stream."""
    o = oracle()
    out = []
    for g in CASES[name]().groups:
        res = [o.chunk_and_hash(p, *g.cfg) for p in g.parts]
        for r in res:
            for x in r:
                x.setflags(write=False)
        out.append(res)
    return out


class Recorded:
    """What check_part asks of an oracle, answered from expected(): the reference is computed once for all the scans that are held to it."""

    def __init__(self, name):
        self.by_id = {}
        for g, res in zip(CASES[name]().groups, expected(name)):
            for p, r in zip(g.parts, res):
                self.by_id[id(p)] = (g.cfg, r)

    def chunk_and_hash(self, data, mn, av, mx):
        cfg, r = self.by_id[id(data)]
        assert cfg == (mn, av, mx)
        return r


# ---- a model of the tile scan's candidates and of the selection, with one rule broken at a time --------------------------------------------
MUTANTS = ("no_halo", "skip_exact", "mask_for_any_d", "general_for_pow2", "qlo_unmasked", "stop_at_masked_run", "one_trip")


def model_candidates(a: np.ndarray, d: int, flags=()) -> np.ndarray:
    """The candidate bits q (cut position q + 1) as k_buzhash_prefix_dma finds them: per 4 KiB wave-tile, the cut test as the necessary
    test on the odd part of d and the exact rotate-and-compare, or the mask test for a power of two."""
    n = len(a)
    if n < WINDOW:
        return np.zeros(0, np.int64)
    h = hashes(a)  # h[q - 47] = H(q + 1)
    q = np.arange(47, n)
    if "no_halo" in flags:  # lane 0, steps k < 47 of a tile: the window's bytes in front of the tile (the halo row) left out
        u = TABLE[a]
        for k in range(47):
            at = q[(q % WTILE == k) & (q >= WTILE)]
            for j in range(k + 1, WINDOW):
                h[at - 47] ^= _rotl_np(u[at - j], j)
    k2 = (d & -d).bit_length() - 1
    dodd = d >> k2
    mask = (is_pow2(d) and "general_for_pow2" not in flags) or "mask_for_any_d" in flags
    if mask:
        hit = (~h & np.uint32(d - 1)) == 0
    else:
        inv = pow(dodd, -1, 1 << 32)
        y = ((h.astype(np.uint64) + 1) * inv & M32).astype(np.uint32)
        necessary = y <= M32 // dodd
        x = y - np.uint32(1 << k2)
        exact = ((x >> np.uint32(k2)) | (x << np.uint32(32 - k2)) if k2 else x) <= M32 // d - 1
        hit = necessary if "skip_exact" in flags else necessary & exact
    return q[hit]


def model_select(cand: np.ndarray, size: int, mn: int, mx: int, flags=()):
    """k_select_cuts over the two-level bitmap of the candidate bits `cand` (ascending): per chunk the flagged 64-byte runs of
    [qlo, qhi] in order, 64 level-1 words a trip; a run's bits below qlo and above qhi masked."""
    runs = np.unique(cand >> 6)
    lens, s = [], 0
    while s < size:
        left = size - s
        if left <= mn:
            length = left
        else:
            end = min(left, mx)
            length = end
            qlo, qhi = s + mn, s + end - 1
            rlo, rhi = qlo >> 6, qhi >> 6
            if qlo <= qhi:
                for r in runs[np.searchsorted(runs, rlo) : np.searchsorted(runs, rhi, side="right")].tolist():
                    if "one_trip" in flags and (r >> 6) >= (rlo >> 6) + 64:
                        break
                    m = cand[np.searchsorted(cand, r << 6) : np.searchsorted(cand, (r << 6) + 64)]
                    if r == rlo and "qlo_unmasked" not in flags:
                        m = m[m >= qlo]
                    if r == rhi:
                        m = m[m <= qhi]
                    if len(m):
                        length = int(m[0]) - s + 1
                        break
                    if "stop_at_masked_run" in flags:
                        break
        lens.append(length)
        s += length
    return np.array(lens, np.uint32)


def model_lengths(a: np.ndarray, cfg, flags=()) -> np.ndarray:
    mn, av, mx = cfg
    return model_select(model_candidates(a, disc(av), flags), len(a), mn, mx, flags)
