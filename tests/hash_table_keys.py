"""Chunk hashes built to collide, wrap and grow in the device hash tables (k_dedup.hip, and the second copy in version_index.hip).

Every one of those tables is open addressing with `mix64(h) & (slots - 1)` as the home slot, linear probing and 0xFFFF...FFFF as the
empty key, whose hash lives in a side word.  mix64 is the murmur3 finaliser, a bijection on 64-bit words, so unmix64 gives a key for
any wanted home slot: key_at(home, j) lands on `home & (S - 1)` in every table of S <= 2^20 slots, and j tells the keys of one home
apart.  The named builders below aim a few hundred such keys at the corners that random hashes at half load never reach.

TableModel is a plain sequential table of the same design.  It PROVES what a case reaches (the longest probe, a probe that steps from
the last slot to slot 0) and, with one rule broken on purpose, that a case would notice that defect
(tests/test_hash_table_keys_cases.py).  It is never the expected value of a GPU result: tests/test_gpu_hash_table_keys.py takes those
from numpy and from the reference library."""
from dataclasses import dataclass, field

import numpy as np

M64 = (1 << 64) - 1
EMPTY = M64  # the tables' empty key: as a hash it is kept in a side word
MUL1, MUL2, SHIFT = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53, 33  # mix64 as the kernels have it
INV1, INV2 = 0x4F74430C22A54005, 0x9CB4B2F8129337DB  # MUL1 * INV1 == MUL2 * INV2 == 1 (mod 2^64)
MIN_SLOTS = 1024
HOME_BITS = 20
FAR = 1 << 30  # first j of the keys that no case ever adds (the absent queries)
PAD_J = 1 << 21  # j of the padding keys


def mix64(z: int) -> int:
    z = ((z ^ (z >> SHIFT)) * MUL1) & M64
    z = ((z ^ (z >> SHIFT)) * MUL2) & M64
    return z ^ (z >> SHIFT)


def unmix64(z: int) -> int:
    z ^= z >> SHIFT  # (self-inverse: the shift is more than half the word)
    z = (z * INV2) & M64
    z ^= z >> SHIFT
    z = (z * INV1) & M64
    return z ^ (z >> SHIFT)


def key_at(home: int, j: int, bits: int = HOME_BITS) -> int:
    """The key whose home slot is `home & (S - 1)` in every table of S <= 2^bits slots; j tells the keys of one home apart."""
    assert 0 <= home < (1 << bits) and 0 <= j < (1 << (64 - bits))
    return unmix64((j << bits) | home)


def keys_at(home: int, js) -> np.ndarray:
    return np.array([key_at(home, int(j)) for j in js], np.uint64)


def slots_for(n: int) -> int:
    """Two slots per hash, a power of two, at least 1024 (include/longtail_hip.h; seen_slots_for in k_dedup.hip)."""
    slots = MIN_SLOTS
    while slots < 2 * n:
        slots <<= 1
    return slots


# ---- the model --------------------------------------------------------------------------------------------------------------------------


class Left(Exception):
    """A probe of the model without the wrap stepped off the end of the array."""


@dataclass
class Walk:
    passed: int = 0  # occupied slots of other keys stepped over
    wrapped: bool = False  # stepped from slot S - 1 to slot 0


class TableModel:
    """Sequential linear probing.  `longest` and `wrapped` are over every operation so far.  The keyword flags each break one rule:
    find_stops (a find gives up at the first slot of another key), no_wrap (slot + 1 without `& mask`: raises Left), reinsert_drops
    (growth drops a pair whose home slot is taken), keep_last (the value of a key is the last one inserted, not the smallest)."""

    def __init__(self, slots: int, **flags):
        assert slots >= MIN_SLOTS and slots & (slots - 1) == 0
        self.slots, self.flags = slots, flags
        self.keys, self.vals = [None] * slots, [None] * slots
        self.side = None  # the value of the EMPTY hash
        self.longest, self.wrapped = 0, False
        self.find_stops, self.no_wrap = flags.get("find_stops", False), flags.get("no_wrap", False)
        self.reinsert_drops, self.keep_last = flags.get("reinsert_drops", False), flags.get("keep_last", False)

    def _step(self, slot: int, walk: Walk) -> int:
        walk.passed += 1
        if slot + 1 == self.slots:
            if self.no_wrap:
                raise Left()
            walk.wrapped = True
        return (slot + 1) & (self.slots - 1)

    def _note(self, walk: Walk) -> Walk:
        self.longest = max(self.longest, walk.passed)
        self.wrapped |= walk.wrapped
        return walk

    def _value(self, old, new, claimed: bool):
        return new if claimed or self.keep_last else min(old, new)

    def insert(self, h: int, v: int):
        """-> (this insert claimed a slot: a new distinct hash, its Walk)"""
        walk = Walk()
        if h == EMPTY:
            claimed = self.side is None
            self.side = self._value(self.side, v, claimed)
            return claimed, walk
        slot = mix64(h) & (self.slots - 1)
        while self.keys[slot] is not None and self.keys[slot] != h:
            slot = self._step(slot, walk)
        claimed = self.keys[slot] is None
        self.keys[slot] = h
        self.vals[slot] = self._value(self.vals[slot], v, claimed)
        return claimed, self._note(walk)

    def find(self, h: int):
        """-> (the value of h, or None where the table does not hold it; the Walk)"""
        walk = Walk()
        if h == EMPTY:
            return self.side, walk
        slot = mix64(h) & (self.slots - 1)
        while True:
            k = self.keys[slot]
            if k == h:
                return self.vals[slot], self._note(walk)
            if k is None or self.find_stops:
                return None, self._note(walk)
            slot = self._step(slot, walk)

    def reinsert_into(self, slots: int) -> "TableModel":
        """Growth: every live pair into a fresh table of `slots`, the side entry carried over.  The new table's `longest` / `wrapped`
        are those of the reinsertion alone."""
        assert slots > self.slots
        new = TableModel(slots, **self.flags)
        new.side = self.side
        for i in range(self.slots):
            h = self.keys[i]
            if h is None:
                continue
            walk, slot = Walk(), mix64(h) & (slots - 1)
            while new.keys[slot] is not None:
                if self.reinsert_drops:
                    slot = None
                    break
                slot = new._step(slot, walk)
            if slot is not None:
                new.keys[slot], new.vals[slot] = h, self.vals[i]
            new._note(walk)
        return new

    def occupied(self) -> np.ndarray:
        return np.array([k is not None for k in self.keys])

    def load(self) -> float:
        return float(self.occupied().sum()) / self.slots


LEFT = "a probe left the array"


def ballot_count(claimed, lane0_only: bool = False) -> int:
    """The distinct count as the insert kernels add it up: one add per wave of 64 of the popcount of the lanes that claimed a slot.
    lane0_only: the defect of a count that looks at lane 0's own claim alone."""
    claimed = [bool(c) for c in claimed]
    waves = [claimed[i : i + 64] for i in range(0, len(claimed), 64)]
    return sum(int(w[0]) if lane0_only else sum(w) for w in waves)


def model_first_seen(calls, slots: int = None, values=None, queries=(), **flags):
    """The arrays of `calls` added one after the other to a table that starts at `slots` (default: the smallest) and grows by the
    sizing rule.  -> dict(answers: the value found for every hash added, distinct: the running count after each call, queries: the
    value of every query (None: absent), tables: the table after each call, grows: the freshly reinserted table of each growth), or
    LEFT when a probe of the no_wrap variant stepped off the array."""
    lane0_only = flags.pop("lane0_only", False)
    t = TableModel(slots or MIN_SLOTS, **flags)
    allh = [int(h) for c in calls for h in c]
    values = list(range(len(allh))) if values is None else [int(v) for v in values]
    distinct, running, tables, grows, pos = 0, [], [], [], 0
    try:
        for c in calls:
            if (pos + len(c)) * 2 > t.slots:
                t = t.reinsert_into(max(t.slots * 2, slots_for(pos + len(c))))
                grows.append(t)
            t = _continue(t)  # (the table after each call is an object of its own, with the figures of that call's inserts)
            claimed =[t.insert(int(h), values[pos + i])[0] for i, h in enumerate(c)]
            distinct += ballot_count(claimed, lane0_only)
            running.append(distinct)
            tables.append(t)
            pos += len(c)
        answers = [t.find(h)[0] for h in allh]
        asked = [t.find(int(q))[0] for q in queries]
    except Left:
        return LEFT
    return dict(answers=answers, distinct=running, queries=asked, tables=tables, grows=grows)


def _continue(grown: TableModel) -> TableModel:
    """A copy of the table to go on with, its counters reset: a freshly grown table keeps the reinsertion's own figures."""
    t = TableModel(grown.slots, **grown.flags)
    t.keys, t.vals, t.side = list(grown.keys), list(grown.vals), grown.side
    return t


# ---- the cases --------------------------------------------------------------------------------------------------------------------------


@dataclass
class Case:
    name: str
    slots: int  # the table size the homes are built for
    hashes: np.ndarray
    corner: str
    queries: list = field(default_factory=list)  # Query objects (absent)
    calls: list = field(default_factory=list)  # grow, lone_claim: the arrays of the add calls
    notes: dict = field(default_factory=dict)


@dataclass
class Query:
    label: str
    key: int
    min_passed: int  # occupied slots the walk steps over before it reaches an empty one
    crosses: bool  # ... and whether it steps from slot S - 1 to slot 0


def _shuffled_repeats(keys: np.ndarray, rng, lo: int = 1, hi: int = 3) -> np.ndarray:
    h = np.repeat(keys, rng.integers(lo, hi + 1, len(keys)))
    rng.shuffle(h)
    return h


def wrap(slots: int = MIN_SLOTS, seed: int = 1) -> Case:
    rng = np.random.default_rng(seed)
    homes = [slots - 3 + i % 3 for i in range(40)] + [i % 2 for i in range(10)]
    keys = np.array([key_at(h, 1 + i) for i, h in enumerate(homes)], np.uint64)
    return Case("wrap", slots, _shuffled_repeats(keys, rng),
                "50 keys with homes S-3 .. S-1 and 0, 1: one cluster from S-3 over the end to slot 46", notes=dict(keys=keys))


def one_home(slots: int = MIN_SLOTS, distinct: int = 300, repeats: int = 150, seed: int = 2) -> Case:
    rng = np.random.default_rng(seed)
    keys = keys_at(slots // 2, range(1000, 1000 + distinct))
    h = np.concatenate([keys, rng.choice(keys, repeats)])
    rng.shuffle(h)
    return Case("one_home", slots, h, f"{distinct} keys of home S/2: probes of up to {distinct - 1} slots", notes=dict(keys=keys))


def half_full_one_home(slots: int = MIN_SLOTS, distinct: int = 512, seed: int = 3) -> Case:
    rng = np.random.default_rng(seed)
    keys = keys_at(slots - 1, range(5000, 5000 + distinct))
    rng.shuffle(keys)
    return Case("half_full_one_home", slots, keys,
                f"{distinct} keys of home S-1: one cluster from S-1 through {distinct - 2}, a probe of {distinct - 1} slots that crosses the end",
                notes=dict(keys=keys))


def specials(slots: int = MIN_SLOTS, seed: int = 1) -> Case:
    h = [int(x) for x in wrap(slots, seed).hashes]
    for pos, value in ((45, 0), (0, EMPTY), (60, 0), (41, EMPTY), (70, EMPTY)):
        h.insert(pos, value)
    h += [0, EMPTY]
    return Case("specials", slots, np.array(h, np.uint64),
                "hash 0 (home 0) and the empty key's hash, each several times, in a cluster that has wrapped onto slot 0")


def cluster_of(hashes, slots: int):
    """(first slot, number of slots, wraps) of the run of occupied slots that crosses the end of a table of `slots` holding `hashes`, or
    of the longest run where none does."""
    t = TableModel(slots)
    for h in np.unique(np.asarray(hashes, np.uint64)):
        t.insert(int(h), 0)
    occ = t.occupied()
    assert not occ.all()
    if occ[slots - 1] and occ[0]:
        first = slots - 1
        while occ[first - 1]:
            first -= 1
        n = 0
        while occ[(first + n) % slots]:
            n += 1
        return first, n, True
    best, run = (0, 0), 0
    for i in range(slots):
        run = run + 1 if occ[i] else 0
        if run > best[1]:
            best = (i - run + 1, run)
    return best[0], best[1], False


def absent_queries(hashes, slots: int, first_j: int = FAR) -> list:
    """Keys that a table of `slots` holding `hashes` lacks, aimed at its cluster (cluster_of): where each walk starts, how many
    occupied slots it must step over to the empty slot that ends it, and whether it crosses the end."""
    first, n, wraps = cluster_of(hashes, slots)
    mask = slots - 1
    mid = n // 2
    out = [Query("the cluster's first slot", key_at(first, first_j), n, wraps),
           Query("the cluster's middle", key_at((first + mid) & mask, first_j + 1), n - mid, wraps and first + mid < slots),
           Query("the empty slot just after the cluster", key_at((first + n) & mask, first_j + 2), 0, False),
           Query("the slot just before the cluster", key_at((first - 1) & mask, first_j + 3), 0, False)]
    if wraps:
        out.append(Query("slot S-1, the cluster wrapped", key_at(mask, first_j + 4), n - (slots - 1 - first), True))
    if EMPTY not in [int(h) for h in hashes]:
        out.append(Query("all-ones before it was ever added", EMPTY, 0, False))
    return out


def absent(slots: int = MIN_SLOTS, seed: int = 1) -> Case:
    w = wrap(slots, seed)
    return Case("absent", slots, w.hashes, "finds of keys the table lacks: walks over a whole wrapped cluster to the empty slot behind it",
                queries=absent_queries(w.hashes, slots))


def absent_keys(home: int, count: int, first_j: int = FAR + 100) -> np.ndarray:
    """`count` keys of one home that no case adds."""
    return keys_at(home, range(first_j, first_j + count))


def padding(hashes, slots: int, count: int) -> np.ndarray:
    """`count` keys that collide nowhere in a table of `slots` holding `hashes`: each alone on its home slot, no two adjacent, three
    free slots away from every occupied one."""
    t = TableModel(slots)
    for h in np.unique(np.asarray(hashes, np.uint64)):
        t.insert(int(h), 0)
    occ = t.occupied()
    near = occ.copy()
    for d in (1, 2, 3):
        near |= np.roll(occ, d) | np.roll(occ, -d)
    homes, last = [], -2
    for s in range(1, slots - 1):  # (slot 0 is hash 0's home, slot S-1 the wrap's)
        if not near[s] and s - last >= 2:
            homes.append(s)
            last = s
    assert len(homes) >= count, (len(homes), count)
    return np.array([key_at(s, PAD_J) for s in homes[:count]], np.uint64)


def padded(case: Case, count: int, seed: int = 7) -> np.ndarray:
    """The case's hashes with padding() mixed in, `count` hashes in all."""
    rng = np.random.default_rng(seed)
    h = np.concatenate([case.hashes, padding(case.hashes, slots_for(count), count - len(case.hashes))])
    rng.shuffle(h)
    return h


GROW_CALLS = {True: (300, 400, 324, 2200, 872), False: (300, 400, 324, 900, 1300, 872)}  # 4096 hashes either way


def grow(skip: bool = True, seed: int = 4) -> Case:
    """Add calls that take a table of 1024 slots to 2048 and on to 8192: in one call that skips 4096 (skip), or by way of 4096."""
    rng = np.random.default_rng(seed)
    end = [key_at(8191, 100 + i) for i in range(12)]  # home S'-1 at every size up to 8192
    same = [key_at(h, 200 + i) for h in (300, 3372, 5000, 777) for i in range(60)]  # all 20 low bits shared: collide at every size
    pairs = []
    for d in (1024, 2048, 4096):  # collide in a table of d slots, split in one of 2 d
        for b in rng.choice(d, 60, replace=False):
            pairs += [key_at(int(b) + off, j) for off in (0, d) for j in (1, 2)]
    filler = [key_at(int(h), 7) for h in rng.choice(1 << HOME_BITS, 2100, replace=False)]
    rest = np.array(end[4:] + same[30:] + pairs + filler, np.uint64)
    rng.shuffle(rest)
    pool = np.concatenate([np.array(end[:4] + same[:30], np.uint64), rest])  # (in from the first call: four keys of home S'-1, 30 of one home)
    calls, used = [], 0
    for n in GROW_CALLS[skip]:
        fresh = int(n * 0.65)
        new = pool[used : used + fresh]
        used += fresh
        c = np.concatenate([new, rng.choice(pool[:used], n - fresh)])
        rng.shuffle(c)
        calls.append(c)
    assert used <= len(pool)
    sizes = [slots_for(t) for t in np.cumsum(GROW_CALLS[skip])]
    return Case("grow", MIN_SLOTS, np.concatenate(calls),
                "1024 -> 2048 -> " + ("" if skip else "4096 -> ") + "8192 slots; pairs that split, keys that still collide, reinserts across the end",
                calls=calls, notes=dict(sizes=sizes))


LONE_N, LONE_P = (1, 63, 64, 65, 256, 257), (0, 62, 63, 64, 255)


def lone_claim(slots: int = MIN_SLOTS) -> Case:
    """calls[0] is the one key that is present already; every later call is n - 1 repeats of it and one new key at position p."""
    home = slots // 4
    present = key_at(home, 9000)
    calls, subs = [np.array([present], np.uint64)], []
    for n in LONE_N:
        for p in sorted({q for q in LONE_P + (n - 1,) if q < n}):
            c = np.full(n, present, np.uint64)
            c[p] = key_at(home, 9001 + len(subs))
            calls.append(c)
            subs.append((n, p))
    return Case("lone_claim", slots, np.concatenate(calls), "one lane of a call claims a slot: lane 0, lane 62, lane 63, the last lane of a partial wave",
                calls=calls, notes=dict(subs=subs))


def cuts_inside(n: int) -> list:
    """Call sizes that cut an array of n hashes inside its clusters: 1, 13, 64 and 65 hashes, then the rest in two halves."""
    sizes = []
    for k in (1, 13, 64, 65):
        if sum(sizes) + k < n:
            sizes.append(k)
    rest = n - sum(sizes)
    return sizes + [rest // 2, rest - rest // 2]


def first_occurrence(h: np.ndarray):
    """numpy's answer: (the index of the first occurrence of every hash, the number of distinct hashes)"""
    _, first, inverse = np.unique(h, return_index=True, return_inverse=True)
    return first[inverse].astype(np.int64), len(first)


def ordinals_for(hashes: np.ndarray, seed: int = 9) -> np.ndarray:
    """A random injection of the positions into [0, 2^31 - 2], some above 2^30, placed so that the smallest ordinal of a hash that
    occurs three times or more is at neither its first nor its last occurrence (and, for those that occur twice, at the first and at
    the last in turn)."""
    rng = np.random.default_rng(seed)
    n = len(hashes)
    o = np.zeros(0, np.int64)
    while len(o) < n:
        o = np.unique(np.concatenate([o, rng.integers(0, 2**31 - 1, 2 * n + 8)]))
    o = rng.permutation(o)[:n]
    twice = 0
    for h in np.unique(hashes):
        at = np.flatnonzero(hashes == h)
        if len(at) < 2:
            continue
        if len(at) >= 3:
            want = at[1 + int(rng.integers(0, len(at) - 2))]
        else:
            want = at[twice % 2 * (len(at) - 1)]
            twice += 1
        low = at[np.argmin(o[at])]
        o[want], o[low] = o[low], o[want]
    return o.astype(np.uint32)


def min_per_hash(hashes: np.ndarray, ordinals: np.ndarray):
    """numpy's answer: (the smallest ordinal among the items with the hash of item j, the number of distinct hashes)"""
    distinct, inverse = np.unique(hashes, return_inverse=True)
    low = np.full(len(distinct), 2**32, np.int64)
    np.minimum.at(low, inverse, ordinals.astype(np.int64))
    return low[inverse], len(low)


# ---- the inputs of the two store-index calls --------------------------------------------------------------------------------------------


def store_index_blob(blocks) -> bytes:
    """A serialized StoreIndex (layout: [version, hash id, blocks, chunks], block hashes, chunk hashes, block chunk offsets, block chunk
    counts, block tags, chunk sizes) of `blocks` = [(block hash, tag, chunk hashes, chunk sizes)]."""
    counts = np.array([len(b[2]) for b in blocks], np.uint32)
    m = int(counts.sum())
    offsets = (np.cumsum(counts) - counts).astype(np.uint32)
    head = np.array([1 << 24, 0x626C6B33, len(blocks), m], np.uint32)
    parts = (head, np.array([b[0] for b in blocks], np.uint64), np.concatenate([np.asarray(b[2], np.uint64) for b in blocks]), offsets, counts,
             np.array([b[1] for b in blocks], np.uint32), np.concatenate([np.asarray(b[3], np.uint32) for b in blocks]))
    return b"".join(a.tobytes() for a in parts)


def store_index_inputs(seed: int = 5):
    """-> (blocks, {name: wanted hashes}) for lthip_get_existing_store_index at 1024 slots.  Wanted: wrap + one_home + specials, with
    duplicates.  Block A (95 % used) holds all-ones and wanted keys; B (25 %) has all-ones as its only wanted chunk, so A's claim keeps
    it out; C (50 %) holds all-ones and one wanted key nobody else has; D (100 %) is wanted through and through, hash 0 included; E
    holds hash 0 among absent keys; F.. draw from the wanted keys with repetition across blocks, absent keys of the cluster's homes and
    of S-1 among them.  Every chunk is 1000 bytes, so a block's usage is its share of wanted chunks."""
    rng = np.random.default_rng(seed)
    S = MIN_SLOTS
    w, o = wrap(S), one_home(S, 300, 40)
    wanted = np.concatenate([specials(S).hashes, o.hashes])
    rng.shuffle(wanted)
    assert len(wanted) <= 512 and len(np.unique(wanted)) < len(wanted)
    wk, ok = w.notes["keys"], o.notes["keys"]
    inside = np.concatenate([absent_keys(S - 3, 8), absent_keys(10, 8), absent_keys(S // 2 + 150, 8), absent_keys(S - 1, 8)])  # in neither set
    lone = ok[-1]  # (a key of the wanted set that only block C holds)
    blocks = [("A", [EMPTY] + list(wk[:12]) + list(ok[:7]) + [inside[0]]),
              ("B", [inside[1], EMPTY, inside[2], inside[3]]),
              ("C", [inside[4], EMPTY, lone, inside[5]]),
              ("D", [0] + list(ok[280:299]) + list(wk[40:50])),
              ("E", [inside[6], 0, inside[7], inside[24]])]
    shared = np.concatenate([wk, ok[:-1]])
    for k in range(10):
        mine = list(rng.choice(shared, 12, replace=False)) + list(rng.choice(inside[8:], 1 + k % 6, replace=False))
        if k % 3 == 0:
            mine.append(EMPTY if k % 2 else 0)
        blocks.append((f"F{k}", [mine[i] for i in rng.permutation(len(mine))]))
    out = [(0x1000 + i, 1 + i % 3, np.array([int(c) for c in chunks], np.uint64), np.full(len(chunks), 1000, np.uint32))
           for i, (_, chunks) in enumerate(blocks)]
    wanted_sets = {"all": wanted, "all-ones not wanted": wanted[wanted != np.uint64(EMPTY)], "all-ones alone": np.full(3, EMPTY, np.uint64)}
    return out, wanted_sets


MISSING_KINDS = ("wrap", "one_home", "half_full_one_home")
MISSING_WHERE = ("store", "version", "both")


def missing_content_inputs(kind: str, where: str, repeats: bool = True, seed: int = 6):
    """-> dict(existing, hashes, sizes, tags, max_block_size, max_chunks_per_block) for lthip_create_missing_content, existing and version
    512 hashes together: the one-shot table has 1024 slots and is exactly half full (by the count it is sized from; the distinct keys
    are fewer).  Store and version share a cluster of `kind`, the version holds keys the store holds and keys it lacks; hash 0 and
    all-ones are in the store, in the version, or in both (`where`).  repeats: the version repeats keys of both sorts -- a list that
    the call's contract (a VersionIndex's unique chunk list) does not cover, see first_occurrences()."""
    rng = np.random.default_rng(seed)
    S, total = MIN_SLOTS, 512
    keys = {"wrap": lambda: wrap(S).notes["keys"], "one_home": lambda: one_home(S).notes["keys"],
            "half_full_one_home": lambda: half_full_one_home(S, 460).notes["keys"]}[kind]()
    keys = keys[rng.permutation(len(keys))]
    held = keys[: len(keys) * 2 // 5]
    lacked = keys[len(held) :]
    both = [np.uint64(0), np.uint64(EMPTY)]
    existing = list(held) + (both if where in ("store", "both") else [])
    version = list(lacked) + list(held[:20])
    if repeats:
        version += list(held[:9]) + list(lacked[:9]) + list(lacked[:4])
    if where in ("version", "both"):
        version += both + (both if repeats else [])
    existing, version = np.array(existing, np.uint64), np.array(version, np.uint64)
    pad = padding(np.concatenate([existing, version]), S, total - len(existing) - len(version))
    existing = np.concatenate([existing, pad[: len(pad) // 3]])  # (padding the store alone holds, padding the version alone brings)
    version = np.concatenate([version, pad[len(pad) // 3 :]])
    rng.shuffle(existing)
    rng.shuffle(version)
    assert len(existing) + len(version) == total
    n = len(version)
    return dict(existing=existing, hashes=version, sizes=rng.integers(1, 131072, n).astype(np.uint32),
                tags=((np.arange(n) * 3 // n) * 7 + 1).astype(np.uint32), max_block_size=262144, max_chunks_per_block=16)


def mostly_repeats_inputs(count: int = 40, seed: int = 12):
    """`count` inputs for lthip_create_missing_content of 1 to 59 version entries drawn from 1 to 29 hashes, the store holding up to 9
    entries drawn from the same hashes."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        n = int(rng.integers(1, 60))
        pool = rng.integers(1, 2**63, int(rng.integers(1, 30)), dtype=np.int64).astype(np.uint64)
        out.append(dict(existing=rng.choice(pool, int(rng.integers(0, 10))), hashes=rng.choice(pool, n),
                        sizes=rng.integers(1, 1000, n).astype(np.uint32), tags=rng.integers(1, 3, n).astype(np.uint32), max_block_size=4096,
                        max_chunks_per_block=4))
    return out


def first_occurrences(inp):
    """The same question with the version as the calls' contract has it: every hash once, where it first occurs, with the size and the
    tag it has there."""
    keep = np.sort(np.unique(inp["hashes"], return_index=True)[1])
    return dict(inp, hashes=inp["hashes"][keep], sizes=inp["sizes"][keep], tags=inp["tags"][keep])


def ref_missing_content(ref, inp) -> bytes:
    """Longtail_CreateMissingContent + Longtail_WriteStoreIndexToBuffer of the reference library on missing_content_inputs()."""
    import ctypes as C

    existing, hashes, sizes, tags = (np.ascontiguousarray(inp[k]) for k in ("existing", "hashes", "sizes", "tags"))
    buf, size = C.c_void_p(), C.c_uint64(0)
    err = ref.dll.refh_missing_content(existing.ctypes.data if len(existing) else None, len(existing), hashes.ctypes.data, sizes.ctypes.data,
                                       tags.ctypes.data, len(hashes), inp["max_block_size"], inp["max_chunks_per_block"], C.byref(buf), C.byref(size))
    assert err == 0, err
    out = bytes((C.c_ubyte * size.value).from_address(buf.value))
    ref.dll.refh_free(buf)
    return out


def store_index_hashes(blob: bytes):
    """(block hashes, chunk hashes) of a serialized StoreIndex"""
    head = np.frombuffer(blob[:16], np.uint32)
    nb, m = int(head[2]), int(head[3])
    return np.frombuffer(blob[16 : 16 + 8 * nb], np.uint64), np.frombuffer(blob[16 + 8 * nb : 16 + 8 * nb + 8 * m], np.uint64)
