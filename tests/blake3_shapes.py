"""The BLAKE3 tree shapes every reducer of k_blake3.hip is pinned at (tests/test_gpu_blake3_shapes.py), as plain tables; checked on the
CPU by tests/test_blake3_shapes_cases.py.

A length is L(n, t) = (n - 1) * 1024 + t: n leaves, t bytes in the last one; L = 0 is one further case, the empty ROOT leaf (n = 1,
t = 0).  A case is (n, t, residue): the range starts at an address with that residue -- modulo 4 for the range calls (the leaf kernel's
realigning loads), modulo 16 for hash_one (vector or byte staging).  All ranges of a table lie, overlapping, in ONE buffer of
SRC_BYTES synthetic bytes (source()), so the bytes behind a range's end are never zero: a last block that is masked one byte short or
long changes the digest."""
from __future__ import annotations

import numpy as np

KIB = 1024
# every residue mod 4 of the last word's mask; a last block of 1, 63 and 64 bytes; one, two and sixteen blocks in the last leaf
TAILS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 961, 1023, 1024)
# every shape of the one-wave reducer (1..64), and the corners of the window reducer up to its limit of 256 leaves
N_SMALL = tuple(range(1, 67)) + (95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256)
# the level reducer: around every power of two up to 4096, and 1537 = 1024 + 512 + 1
N_BIG = (257, 258, 511, 512, 513, 1023, 1024, 1025, 1537, 2047, 2048, 2049, 4097)
N_LEVEL = (1, 2, 3, 5, 64, 65, 256) + N_BIG
N_ONE = tuple(range(1, 65))
RANGE_RESIDUES = (0, 1, 2, 3)  # mod 4
ONE_RESIDUES = (0, 1, 4, 8, 15)  # mod 16
ONE_PINNED_RESIDUES = (0, 1)
WINDOW_MAX_LEN = 256 * KIB  # lthip_hash_ranges takes the window reducer for 0 < max_len <= this
PW = 1024  # leaf slots of a window (k_blake3.hip)

SRC_SEED, SRC_KIND = 0xB3, 0
SRC_BYTES = 4097 * KIB + 64  # the longest range at any residue; the callers pad the allocation by a further 64 bytes
SRC_PAD = 64

# runs of 64-bit values (lthip_hash_runs_u64[_bounded]): 32768 values are 256 KiB, the window reducer's limit
RUN_VALUES = (0, 1, 127, 128, 129, 1023, 1024, 32767, 32768)

# the stream reducer: batches of 1 MiB below the tail; B gives every popcount / trailing-zero pattern of a stack up to depth 4
STREAM_BATCH = 1 << 20
STREAM_B = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17)
STREAM_TAILS = (1, 1023, 1024, 1025, 3 * KIB + 5, 5 * KIB, 6 * KIB + 64, 7 * KIB + 1)
STREAM_EDGES = ((0, STREAM_BATCH), (3, STREAM_BATCH - 1), (7, STREAM_BATCH))
STREAM_BYTES = 18 * STREAM_BATCH

# the fused call: every chunk of a (m, m, m) configuration is m bytes, the last of a part the remainder
FUSED_M = {1024: 700, 1025: 700, 3072: 400, 3073: 400, 65537: 20}  # m -> q: parts of q * m, q * m + 1 and q * m + m - 1 bytes
FUSED_LEVEL = (300000, (1 << 20) + 5)  # above the window limit: (m, part size)

STRADDLE_S = (767, 768, 769, 1022, 1023, 1024, 1025)


def length(n: int, t: int) -> int:
    return (n - 1) * KIB + t


def leaves(nbytes: int) -> int:
    return max(1, (nbytes + KIB - 1) // KIB)


def source(oracle) -> np.ndarray:
    """The SRC_BYTES + SRC_PAD bytes all tables read (the pad keeps the aligned dword of a range's last byte inside the allocation)."""
    return oracle.synth(SRC_BYTES + SRC_PAD, SRC_SEED, SRC_KIND)


def _start(index: int, nbytes: int, residue: int, modulus: int) -> int:
    """A start with the residue modulo 4 or 16, spread over the room the length leaves in the source."""
    room = (SRC_BYTES - nbytes - modulus) // modulus
    return (index * 7919 % (room + 1)) * modulus + residue


def _cases(shapes, residues_of, modulus):
    """-> [(n, t, residue)], (offsets u64, lens u32)"""
    cases = [(n, t, r) for i, (n, t) in enumerate(shapes) for r in residues_of(i)]
    lens = np.array([length(n, t) for n, t, _ in cases], np.uint32)
    offs = np.array([_start(i, int(l), r, modulus) for i, ((_, _, r), l) in enumerate(zip(cases, lens))], np.uint64)
    return cases, offs, lens


def _shapes(ns):
    return [(n, t) for n in ns for t in TAILS]


def small_table():
    """The window reducer's table: the empty range and N_SMALL x TAILS, each at every residue mod 4."""
    return _cases([(1, 0)] + _shapes(N_SMALL), lambda i: RANGE_RESIDUES, 4)


def level_table():
    """The level reducer's table: N_LEVEL x TAILS.  The residue cross is thinned for the 236 MiB of N_BIG: shape number i takes the one
    residue i mod 4 (14 tails per n: every n meets every residue), the shapes of n <= 256 take all four."""
    shapes = [(1, 0)] + _shapes(N_LEVEL)
    return _cases(shapes, lambda i: RANGE_RESIDUES if shapes[i][0] <= 256 else (RANGE_RESIDUES[i % 4],), 4)


def one_table(residues=ONE_RESIDUES):
    """hash_one's table: lengths 0 and 65536 and N_ONE x TAILS (65536 = L(64, 1024) is one of them), at each residue mod 16."""
    return _cases([(1, 0)] + _shapes(N_ONE), lambda i: residues, 16)


def stream_cases():
    """[(B, tail bytes)]: the empty stream, the full cross of the sweep (650 MiB for the oracle, under two seconds) and the full-batch
    edges."""
    return [(0, 0)] + [(B, tail) for B in STREAM_B for tail in STREAM_TAILS] + list(STREAM_EDGES)


def run_sets():
    """Run tables for lthip_hash_runs_u64: [(name, first u32[runs + 1])] over the source viewed as 64-bit values.  Runs are consecutive,
    so the table's lengths that are a multiple of 8 (t = 64, 128, 1024) go one tail per set, and RUN_VALUES make a set of their own."""
    # (a run of n values is (n, t, residue) = (leaves of 8 n bytes, bytes of the last leaf, 0))
    sets = []
    lens = [v for _ in range(3) for v in RUN_VALUES] + [v for v in reversed(RUN_VALUES)]
    sets.append(("values", lens))
    for t in TAILS:
        if t % 8 == 0:
            sets.append((f"t{t}", [0] + [length(n, t) // 8 for n in N_SMALL]))
    # runs of at most 16384 values: with both bounds DOUBLED the longest run is still within the window reducer's 256 KiB
    sets.append(("half", [v for v in RUN_VALUES if v <= 16384] + [length(n, 64) // 8 for n in N_SMALL if n <= 128]))
    out = []
    for name, ls in sets:
        first = np.concatenate([[0], np.cumsum(ls)]).astype(np.uint32)
        assert int(first[-1]) * 8 <= SRC_BYTES
        out.append((name, first))
    return out


def batch(shapes):
    """A batch of its own from [(n, t)]: range i starts at residue i mod 4."""
    return _cases(shapes, lambda i: (RANGE_RESIDUES[i % 4],), 4)


def _one_leaf(count, every_fourth_empty=False):
    return [(1, 0) if every_fourth_empty and i % 4 == 3 else (1, TAILS[i % len(TAILS)]) for i in range(count)]


def _mixed(total_leaves):
    """Ranges of 1, 2, 3, 5, 8, ... 55 leaves in turn that sum to exactly total_leaves."""
    out, left, i = [], total_leaves, 0
    while left:
        n = min(left, (1, 2, 3, 5, 8, 13, 21, 34, 55)[i % 9])
        out.append((n, TAILS[i % len(TAILS)]))
        left -= n
        i += 1
    return out


def window_scenarios():
    """{name: [(n, t)]}: deterministic batches for the window reducer (PW = 1024 leaf slots per window, ranges of at most 256 leaves; a
    window owns the ranges whose FIRST slot lies in it).
      straddle_s   s one-leaf ranges, a 256-leaf range, 300 one-leaf ranges: the large range ends at the window's boundary (s = 768),
                   starts on the window's last slot (1023) or on the first slot of the next (1024: the first window then ends with
                   its own ranges, the second starts with one)
      the two ways the kernel fills its per-slot table, chosen by ranges * 8 < slots: 4 x 256 and 113 x 9 take the first, 1024 x 1
      (every fourth empty), 128 x 8 (equality) and 146 x 7 the second
      totals of exactly two windows, two windows and one slot, one range, one empty range"""
    sc = {f"straddle_{s}": _one_leaf(s) + [(256, TAILS[s % len(TAILS)])] + _one_leaf(300) for s in STRADDLE_S}
    sc["4x256"] = [(256, t) for t in (1, 1023, 1024, 64)]
    sc["1024x1_every_fourth_empty"] = _one_leaf(1024, True)
    sc["128x8"] = [(8, TAILS[i % len(TAILS)]) for i in range(128)]
    sc["113x9"] = [(9, TAILS[i % len(TAILS)]) for i in range(113)]
    sc["146x7"] = [(7, TAILS[i % len(TAILS)]) for i in range(146)]
    sc["total_2048"] = _mixed(2048)
    sc["total_2049"] = _mixed(2049)
    sc["one_range"] = [(37, 961)]
    sc["one_empty_range"] = [(1, 0)]
    return sc


def what(cases, i) -> str:
    n, t, r = cases[i]
    return f"(n={n}, t={t}, residue={r}, position {i} of {len(cases)})"


def first_mismatch(got, exp, cases, order=None) -> str:
    """'' when equal, else the first differing case named as (n, t, residue, position in the batch)."""
    bad = np.nonzero(np.asarray(got) != np.asarray(exp))[0]
    if len(bad) == 0:
        return ""
    p = int(bad[0])
    i = p if order is None else int(order[p])
    n, t, r = cases[i]
    return f"{len(bad)} of {len(exp)} digests differ, first (n={n}, t={t}, residue={r}, position {p} in the batch): " \
           f"got {int(got[p]):016x}, expected {int(exp[p]):016x}"
