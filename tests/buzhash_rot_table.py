"""Bytes for the Buzhash scans' table of rotations, and a numpy model of a scan that reads one (CPU, numpy only).

The scans of k_buzhash.hip look the byte at run position j up in R[j mod 32][b] = rotr(T[b], j mod 32), at LDS dword (j mod 32) * 256 + b:
a wrong word, a wrong row for r = 31 or a wrong rotation of the halo word shows only where the cut test sees the hash, so the parts here
are small-parameter ones on which the chunk list depends on every entry.
  part A    256 KiB of seeded random bytes: every (byte value, position mod 32) pair occurs at least 8 times;
  parts B   64 KiB drawn from the eight values c, c + 32, ..., c + 224 of one LDS bank (c = 0 and c = 31): the worst conflict pattern;
  part C    64 KiB of one byte with 4 KiB of random bytes in the middle: every lane on one address, then conflicts.
tests/test_buzhash_rot_table_cases.py proves what the parts reach, tests/test_gpu_buzhash_rot_table.py runs them through the scans."""
from __future__ import annotations

import functools

import numpy as np

from tests import buzhash_plants as P

SEED = 20261021
KIB = 1 << 10
CFGS = [(64, 128, 4096), (64, 86, 300)]  # d = 96, and the power of two 64 (both from tests/test_gpu_chunk_walk.py's CFGS)
HEADLINE = (8192, 32768, 131072)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def parts():
    """name -> bytes, made once and read-only."""
    rng = np.random.default_rng(SEED)
    out = {"A": rng.integers(0, 256, 256 * KIB, dtype=np.uint8)}
    for c in (0, 31):
        out[f"B{c}"] = (c + 32 * rng.integers(0, 8, 64 * KIB)).astype(np.uint8)
    c = np.full(64 * KIB, 0xA7, np.uint8)
    c[30 * KIB : 34 * KIB] = rng.integers(0, 256, 4 * KIB, dtype=np.uint8)
    out["C"] = c
    return {k: _frozen(v) for k, v in out.items()}


def rot_table() -> np.ndarray:
    """R[r][v] = rotr(T[v], r): the table prefix_table_init writes."""
    t = P.TABLE
    return np.stack([t if r == 0 else (t >> np.uint32(r)) | (t << np.uint32(32 - r)) for r in range(32)])


def pair_counts(a: np.ndarray) -> np.ndarray:
    """[r][v]: how often byte v stands at a position that is r modulo 32."""
    n = np.zeros((32, 256), np.int64)
    np.add.at(n, (np.arange(len(a)) % 32, a), 1)
    return n


def model_candidates(a: np.ndarray, d: int, table: np.ndarray) -> np.ndarray:
    """The candidate bits q (cut position q + 1) of a scan that takes U[q] = table[q mod 32][a[q]] and never rotates a table word:
    H(p) = rotl(XOR of U[p-48 .. p-1], (p - 1) mod 32)."""
    n = len(a)
    if n < P.WINDOW:
        return np.zeros(0, np.int64)
    pre = np.zeros(n + 1, np.uint32)
    np.bitwise_xor.accumulate(table[np.arange(n) % 32, a], out=pre[1:])
    q = np.arange(47, n)
    w = pre[q + 1] ^ pre[q - 47]
    r = (q % 32).astype(np.uint32)
    h = (w << r) | (w >> ((np.uint32(32) - r) & np.uint32(31)))  # (r == 0: w | w)
    return q[h % np.uint32(d) == np.uint32(d - 1)]


def select(cand: np.ndarray, size: int, mn: int, mx: int) -> np.ndarray:
    """Chunk lengths from the candidate bits: the first candidate q in [start + mn, start + min(left, mx) - 1] ends the chunk behind q."""
    lens, s = [], 0
    while s < size:
        left = size - s
        length = left if left <= mn else min(left, mx)
        if left > mn:
            i = int(np.searchsorted(cand, s + mn))
            if i < len(cand) and cand[i] <= s + length - 1:
                length = int(cand[i]) - s + 1
        lens.append(length)
        s += length
    return np.array(lens, np.uint32)


def model_lengths(a: np.ndarray, cfg, table: np.ndarray) -> np.ndarray:
    mn, av, mx = cfg
    return select(model_candidates(a, P.disc(av), table), len(a), mn, mx)
