"""Hand-built SOURCES for the LZ4 encoder (k_lz4.hip and lz4/*.inc), each named for the corner of the block format or of the parser it
holds, and the batch lists that put blocks of different routes into one call.  Pure numpy, deterministic; nothing here loads a library.
tests/test_lz4_encoder_sources_cases.py proves the table on the CPU (with the oracle's greedy parse), tests/test_gpu_lz4_encoder_sources.py
runs it on the GPU.

"noise" is seeded default_rng bytes, mended until no four bytes stand twice within 65 535 bytes (gram_repeats): whatever a parser finds
in a source is what the source was given on purpose.  The numbers the encoder is built around are named once, below; source_constants()
reads them back from the kernel source.

What the GPU parser needs to SEE a repeat, and what the table does about it (read off lz4_classify.inc and lz4_lane_parse.inc):
  - the classification pass hands a 32 KiB half-group to the lane parser only if one of its units repeats four bytes inside the first
    640 bytes it probes (64 positions at strides 1, 2, 3, 4, a private and at first empty table); otherwise the half is skimmed and a
    lone far repeat is never looked at.  `A | A[:32]` at a unit's first byte is such a repeat (positions 64, 66, .. find 0, 2, ..): the
    sources that do not begin that way anyway exist a second time behind a BEACON unit that does.
  - history enters the lane parser's tables at aligned dwords only, and a lane probes single bytes for four steps at its sub-unit's
    first byte and behind a match, aligned dwords otherwise: a repeat whose distance is a multiple of four is found at its first
    byte (up to 3 bytes late, 8 are recovered backwards), another one only from a sub-unit's first bytes.  The sources marked
    "distance % 4 == 0" copy from A[k:] with the k that makes their distance one; the others keep the plain form (the reference's
    greedy parse takes either)."""
from __future__ import annotations

import functools
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

U = 4096              # the unit (segment_log2 = 12)
G_BATCH, G_LANES = 8, 16
H = G_BATCH * U       # a classification group, half a lane-parser group
G = G_LANES * U       # a lane-parser group: the window a match can reach back in
SUB = 64              # a lane's sub-unit
LANE_EXT = 36         # a lane extends a match this far on its own, the wave takes over beyond
REACH = 65535         # the largest offset the format holds
SEGMENT_LOG2 = 12

EXPECTED_CONSTANTS = dict(SEGMENT_LOG2=SEGMENT_LOG2, G_BATCH=G_BATCH, G_LANES=G_LANES, SUB=SUB, SUB_STATED=SUB, LANE_EXT=LANE_EXT,
                          LANE_EXT_PARSE=LANE_EXT)


def source_constants(csrc: Path) -> dict:
    """The same numbers as k_lz4.hip and its parts state them: the default unit, the two group sizes, the lanes per unit (a unit is
    handed to the lane parse as sub_bytes >> 6 bytes per lane) and, from the comments that state them as numbers, the sub-unit and the
    lane's own extension.  An assertion or a wrong value means the kernel was retuned and the table stands beside its boundaries."""
    main = (csrc / "k_lz4.hip").read_text()
    lanes = (csrc / "lz4" / "lz4_lanes_kernel.inc").read_text()
    parse = (csrc / "lz4" / "lz4_lane_parse.inc").read_text()

    def one(pattern, text, where):
        m = re.search(pattern, text)
        assert m, f"{where} no longer says /{pattern}/"
        return int(m[1])

    return dict(SEGMENT_LOG2=one(r"if \(segment_log2 == 0\)\s+segment_log2 = (\d+);", main, "k_lz4.hip"),
                G_BATCH=one(r"constexpr int LZ4_G_BATCH = (\d+);", main, "k_lz4.hip"),
                G_LANES=one(r"constexpr int LZ4_G_LANES = (\d+);", main, "k_lz4.hip"),
                SUB=U >> one(r"start_limit, end_limit, sub_bytes >> (\d+), out", lanes, "lz4_lanes_kernel.inc"),
                SUB_STATED=one(r"every LANE owns a (\d+)-byte sub-unit", main, "k_lz4.hip"),
                LANE_EXT=one(r"forwards (\d+) bytes on its own", main, "k_lz4.hip"),
                LANE_EXT_PARSE=one(r"one more 16-byte round of their own \(at most (\d+) bytes\)", parse, "lz4_lane_parse.inc"))


# ---- bytes ---------------------------------------------------------------------------------------------------------------------------

def gram_repeats(a: np.ndarray, reach: int = REACH) -> np.ndarray:
    """the positions p whose four bytes also stand at a q with p - reach <= q < p, ascending"""
    if len(a) < 5:
        return np.zeros(0, np.int64)
    b = a.astype(np.uint32)
    g = b[:-3] | (b[1:-2] << np.uint32(8)) | (b[2:-1] << np.uint32(16)) | (b[3:] << np.uint32(24))
    order = np.argsort(g, kind="stable")  # equal grams stay in position order: a pair within reach shows as a neighbouring pair
    gs = g[order]
    hit = (gs[1:] == gs[:-1]) & (order[1:] - order[:-1] <= reach)
    return np.sort(order[1:][hit])


@functools.lru_cache(maxsize=None)
def _noise(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    for _ in range(64):
        r = gram_repeats(a)
        if r.size == 0:
            break
        a[r] = rng.integers(0, 256, r.size, dtype=np.uint8)
    assert gram_repeats(a).size == 0
    a.setflags(write=False)
    return a


def noise(n: int, seed: int) -> np.ndarray:
    """n bytes without a 4-byte repeat within reach (a fresh copy)"""
    return _noise(n, seed).copy()


def cat(*parts) -> np.ndarray:
    return np.concatenate([np.asarray(p, np.uint8) for p in parts]) if parts else np.zeros(0, np.uint8)


def periodic(period_bytes: np.ndarray, n: int) -> np.ndarray:
    p = len(period_bytes)
    return np.tile(period_bytes, n // p + 1)[:n].copy() if n else np.zeros(0, np.uint8)


def text(n: int, seed: int) -> np.ndarray:
    """word soup: 48 words of 2 .. 9 lower-case letters, drawn at random, one space between them"""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 10)), dtype=np.uint8)) + b" " for _ in range(48)]
    out, have = [], 0
    while have < n:
        w = words[int(rng.integers(0, 48))]
        out.append(w)
        have += len(w)
    return np.frombuffer(b"".join(out), np.uint8)[:n].copy()


def differ(a: np.ndarray, i: int, value: int) -> None:
    """a[i] != value: a match that is meant to stop (or to begin) at a[i] does"""
    if 0 <= i < len(a) and int(a[i]) == int(value):
        a[i] ^= 0x55


def beacon_unit(seed: int) -> np.ndarray:
    """a unit the classification pass sees redundancy in: B | B[:32] | noise"""
    b = noise(U, seed)
    b[SUB : SUB + 32] = b[:32]
    differ(b, SUB + 32, b[32])
    return b


# ---- the table -----------------------------------------------------------------------------------------------------------------------

Source = namedtuple("Source", "name family data short_period")  # short_period: period <= 8 and at least one unit long (the ratio floor)
FAMILIES = ("block end", "literal run", "stitch steps", "match length", "periods and offsets", "unit mix")

BLOCK_END_LENGTHS = list(range(30)) + [x + d for x in (U, H, G) for d in range(-6, 18)]
END_GAPS = (0, 4, 5, 6, 11, 12, 13)
LIT_RUNS = list(range(13, 18)) + list(range(268, 273)) + list(range(523, 528)) + [15 + 255 * 16 - 1, 15 + 255 * 16, 15 + 255 * 16 + 1]
SEAM_SUMS = (14, 15, 16, 269, 270, 271)
SEAM_CARRIES = (1, 14, 15, 255, 269)
MATCH_LENGTHS = [4, 5] + list(range(17, 22)) + list(range(35, 39)) + list(range(272, 277)) + list(range(527, 532))
SHORT_PERIODS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65)
LONG_PERIODS = (U - 1, U, U + 1, H - 1, H, H + 1, G - 2, G - 1, G, G + 1, 2 * G - 1, 2 * G)
FAR_IN_GROUP = (65000, 65300)  # offsets the lane parser can reach: both ends inside one group


def _block_end(add):
    pats = (("constant", np.array([0x41], np.uint8)), ("period 3", noise(3, 11)), ("period 7", noise(7, 12)))
    for label, pat in pats:
        for n in BLOCK_END_LENGTHS:
            add(f"block end: {label}, {n} bytes", "block end", periodic(pat, n), short_period=n >= U)
    base = _noise(G + 32, 13)
    for n in BLOCK_END_LENGTHS:
        for gap in END_GAPS:
            a = base[:n].copy()
            r = min(40, (n - gap) // 2)
            if r >= 4:
                e = n - gap
                a[e - r : e] = a[e - 2 * r : e - r]
                differ(a, e, a[e - r])              # the repeat ends where the table says
                if e - 2 * r - 1 >= 0:
                    differ(a, e - r - 1, a[e - 2 * r - 1])  # ... and begins there
            where = "to the end" if gap == 0 else f"ending {gap} bytes before the end"
            add(f"block end: noise of {n} bytes, the {r if r >= 4 else 0} bytes {where} repeat the ones before", "block end", a)


def _lit_run_piece(L, seed, start, aligned):
    """A | A[:32] | noise(L) | A[k : k + 40] | noise(9), placed at `start` of its source (a multiple of 4).  aligned: k makes the
    second match's distance a multiple of four"""
    A = noise(SUB, seed)
    N = noise(L, seed + 1)
    T = noise(9, seed + 2)
    k = (start + SUB + 32 + L) % 4 if aligned else 0
    differ(N, 0, A[32])
    if k:
        differ(N, L - 1, A[k - 1])
    differ(T, 0, A[k + 40])
    return cat(A, A[:32], N, A[k : k + 40], T)


def _seam(carry, mid_units, first, seed):
    """A | A[:32] | noise | A[j : j + 32] ending `carry` bytes before unit 0's end | noise: carry + mid_units whole units + first bytes
    | A[k : k + 40] | noise(9): the literal run between the last two matches crosses one unit seam or several.  Both distances are
    multiples of four."""
    A = noise(SUB, seed)
    s1 = U - carry - 32
    j = s1 % 4
    s2 = U + mid_units * U + first
    k = s2 % 4
    a = noise(s2 + 40 + 9, seed + 1)
    a[:SUB] = A
    a[SUB : SUB + 32] = A[:32]
    differ(a, SUB + 32, A[32])
    a[s1 : s1 + 32] = A[j : j + 32]
    differ(a, s1 - 1, A[j - 1] if j else a[s1 - 1] ^ 0x55)
    differ(a, s1 + 32, A[j + 32])
    a[s2 : s2 + 40] = A[k : k + 40]
    if k and s2 - 1 != s1 + 32:
        differ(a, s2 - 1, A[k - 1])
    differ(a, s2 + 40, A[k + 40])
    return a


def _literal_runs(add):
    for L in LIT_RUNS:
        add(f"literal run: A | A[:32] | noise({L}) | A[:40] | noise(9)", "literal run", _lit_run_piece(L, 1000 + 3 * L, 0, False))
        if L % 4:
            add(f"literal run: the same with {L} literals, distance % 4 == 0", "literal run", _lit_run_piece(L, 1000 + 3 * L, 0, True))
    for total in SEAM_SUMS:
        for carry in SEAM_CARRIES:
            if carry <= total:
                add(f"literal run: {total} literals over a unit seam, {carry} + {total - carry}", "literal run",
                    _seam(carry, 0, total - carry, 3000 + 16 * total + carry))
    for mid in (1, 2, 3):
        for carry in (1, 15, 255):
            exact = (15 - carry - mid * U) % 255  # carry + mid * U + exact = 15 + 255 k
            for first in sorted({max(exact - 1, 0), exact, exact + 1}):
                total = carry + mid * U + first
                add(f"literal run: {total} literals through {mid} match-less units, {carry} + {mid} x {U} + {first}", "literal run",
                    _seam(carry, mid, first, 5000 + 64 * mid + carry + 1000 * first))


def _steps_block(units, seed, starts, repeat_unit0=()):
    """`units` units of noise; a unit of `starts` begins with B | B[:32] (its one match); a unit of repeat_unit0 is unit 0 again"""
    a = noise(units * U, seed)
    for i, u in enumerate(starts):
        o = u * U
        a[o + SUB : o + SUB + 32] = a[o : o + 32]
        differ(a, o + SUB + 32, a[o + 32])
    for u in repeat_unit0:
        a[u * U : (u + 1) * U] = a[:U]
    return a


def _stitch_steps(add):
    add("stitch steps: 70 units, a match in unit 0, units 1 .. 66 noise, units 67 .. 69 repeat unit 0", "stitch steps",
        _steps_block(70, 21, (0,), (67, 68, 69)))
    add("stitch steps: 66 units, matches in units 0 and 63 only", "stitch steps", _steps_block(66, 22, (0, 63)))
    add("stitch steps: 66 units, matches in units 0 and 64 only", "stitch steps", _steps_block(66, 23, (0, 64)))
    add("stitch steps: 70 units, a match in the last unit only", "stitch steps", _steps_block(70, 24, (69,)))
    add("stitch steps: 130 units of noise", "stitch steps", noise(130 * U, 25))


def _match_piece(m, seed, start, k, tail=30):
    """A(600) | noise | A[k : k + m] | noise(tail), the match at `start` of the piece"""
    A = noise(600, seed)
    a = noise(start + m + tail, seed + 1)
    a[:600] = A
    a[start : start + m] = A[k : k + m]
    differ(a, start - 1, A[k - 1] if k else a[start - 1] ^ 0x55)
    differ(a, start + m, A[k + m])
    return a


def _match_lengths(add):
    for m in MATCH_LENGTHS:
        plain = _match_piece(m, 7000 + 5 * m, 620, 0)
        add(f"match length: A(600) | noise(20) | A[:{m}] | noise(30)", "match length", plain)
        add(f"match length: the same with {m} bytes behind a beacon unit", "match length", cat(beacon_unit(7001 + 5 * m), plain))
        # the match's last byte at a sub-unit's last byte, at the unit's last byte, and its end 1 and 8 bytes past the unit's
        for what, end, tail in (("a sub-unit's last byte", 1280, 30), ("the unit's last byte", U, 30), ("one byte past the unit's end", U + 1, 30),
                                ("8 bytes past the unit's end", U + 8, 30)):
            s = end - m
            add(f"match length: {m} bytes ending at {what}", "match length", cat(beacon_unit(7002 + 5 * m), _match_piece(m, 7000 + 5 * m, s, s % 4, tail)))
        for b in range(1, 9):
            s = 1280 + b
            add(f"match length: {m} bytes starting {b} bytes after a sub-unit's first byte", "match length",
                cat(beacon_unit(7003 + 5 * m), _match_piece(m, 7000 + 5 * m, s, s % 4)))
    for m in (19, 274):
        for b in range(1, 9):
            s = 1280 - b
            add(f"match length: {m} bytes starting {b} bytes before a sub-unit's first byte", "match length",
                cat(beacon_unit(7004 + 5 * m), _match_piece(m, 7000 + 5 * m, s, s % 4)))


def _periods(add):
    for p in SHORT_PERIODS:
        add(f"period {p} over 9000 bytes", "periods and offsets", periodic(noise(p, 30 + p) if p > 1 else np.array([0], np.uint8), 9000), short_period=p <= 8)
    for p in LONG_PERIODS:
        add(f"period {p} over two periods + 5000 bytes", "periods and offsets", periodic(noise(p, 40000 + p), 2 * p + 5000))
    add("nothing repeats: noise(G) | noise'(G)", "periods and offsets", noise(2 * G, 51))
    for back in (G, G - 1):
        a = noise(2 * G + 200, 52 + back)
        a[back + 300 : back + 400] = a[300:400]
        add(f"the only repeat lies {back} back", "periods and offsets", a)
    for d in FAR_IN_GROUP:
        a = cat(beacon_unit(60 + d), noise(H - U, 61 + d), beacon_unit(62 + d), noise(H - U, 63 + d))
        a[128 + d : 128 + d + 64] = a[128 : 128 + 64]
        differ(a, 128 + d - 1, a[127])
        differ(a, 128 + d + 64, a[128 + 64])
        add(f"offset {d} inside one group", "periods and offsets", a)


def _unit_mix(add):
    nz, tx = noise(G, 71), text(G, 72)
    a = nz.copy()
    for u in range(1, 16, 2):
        a[u * U : (u + 1) * U] = tx[u * U : (u + 1) * U]
    add("unit mix: 16 units, noise and text in turns", "unit mix", a)
    add("unit mix: a noise half, then a text half", "unit mix", cat(nz[:H], tx[:H]))
    add("unit mix: a text half, then a noise half", "unit mix", cat(tx[:H], nz[:H]))


@functools.lru_cache(maxsize=None)
def sources():
    out, names = [], set()

    def add(name, family, data, short_period=False):
        assert name not in names and family in FAMILIES, name
        names.add(name)
        data = np.ascontiguousarray(data, np.uint8)
        data.setflags(write=False)
        out.append(Source(name, family, data, short_period))

    for build in (_block_end, _literal_runs, _stitch_steps, _match_lengths, _periods, _unit_mix):
        build(add)
    return tuple(out)


def by_name(name: str) -> Source:
    return next(s for s in sources() if s.name == name)


# ---- coverage: the table cannot pass by missing its corners ---------------------------------------------------------------------------

class Coverage:
    """The union of loose() over the payloads of the table, and the conditions it has to meet: every field boundary the table is built
    for is in some payload.  The same conditions for the oracle's payloads (CPU) and for the GPU's."""

    LIT_LENS = (14, 15, 16, 269, 270, 271)
    MATCH_LENS = (18, 19, 20, 273, 274, 275)

    def __init__(self):
        self.lit_lens, self.match_lens, self.offsets = set(), set(), set()
        self.ends_at_5, self.starts_at_12, self.zero_offset = [], [], []

    def add(self, source: Source, fields) -> None:
        n = len(source.data)
        for e in fields:
            if "ll" in e:
                self.lit_lens.add(e["ll"])
            if e["off"] is None or e["ml"] is None:
                continue
            self.match_lens.add(e["ml"])
            self.offsets.add(e["off"])
            start = e["op"] + e["ll"]
            if e["off"] == 0:
                self.zero_offset.append(source.name)
            if start + e["ml"] == n - 5:
                self.ends_at_5.append(source.name)
            if start == n - 12:
                self.starts_at_12.append(source.name)

    def missing(self) -> list:
        out = [f"literal length {v}" for v in self.LIT_LENS if v not in self.lit_lens]
        out += [f"match length {v}" for v in self.MATCH_LENS if v not in self.match_lens]
        out += [f"offset {v}" for v in (1, 2, 3) if v not in self.offsets]
        if not any(v >= 65000 for v in self.offsets):
            out.append("an offset of 65 000 and more")
        if not any(v >= 64 * U for v in self.lit_lens):
            out.append("a literal length of 64 units and more")
        if not self.ends_at_5:
            out.append("a match that ends exactly at raw_len - 5")
        if not self.starts_at_12:
            out.append("a match that starts exactly at raw_len - 12")
        if self.zero_offset:
            out.append(f"no offset field is 0 (found in {self.zero_offset[:3]})")
        return out


# ---- batches: blocks of every route in one call -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def batch_blocks():
    """the distinct blocks of the batch lists: (name, data); an empty block and a block of 1, 12 and 13 bytes (the 13 bytes constant: the
    shortest source that may hold a match), a block without a match (the route the match finder lays out on its own), a matched block
    and the 70-unit block"""
    one = lambda n: by_name(n).data
    return (("empty", np.zeros(0, np.uint8)), ("1 byte", noise(1, 81)), ("12 bytes", np.full(12, 0x42, np.uint8)), ("13 bytes", np.full(13, 0x43, np.uint8)),
            ("no match, 3 units + 7", noise(3 * U + 7, 82)), ("matched: text", text(5 * U + 123, 83)),
            ("the 70-unit block", one("stitch steps: 70 units, a match in unit 0, units 1 .. 66 noise, units 67 .. 69 repeat unit 0")))


def batches():
    """name -> the indices into batch_blocks() of one call"""
    n = len(batch_blocks())
    base = list(range(n))
    return {"as listed": base, "reversed": base[::-1], "every block doubled": [i for i in base for _ in (0, 1)]}
