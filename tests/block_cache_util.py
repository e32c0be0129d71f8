"""A Python model of longtail_amd/csrc/block_cache.h, the bookkeeping of the device cache of decoded blocks (include/longtail_hip.h, "a
cache of decoded blocks"): slots that are free, reserved or visible, pins, strict LRU by one counter.  The sanitizer test replays the same
operations through the header and compares the state after every one; the GPU tests predict `contains` with it."""

NO_SLOT = -1
FREE, RESERVED, VISIBLE = "F", "R", "V"
M64 = (1 << 64) - 1


def table_digest(chunk_hashes, chunk_sizes):
    """FNV-1a over per chunk its hash (8 bytes, little end first) and its size (4 bytes)."""
    h = 0xCBF29CE484222325
    for ch, cs in zip(chunk_hashes, chunk_sizes):
        for v, n in ((int(ch), 8), (int(cs), 4)):
            for i in range(n):
                h = ((h ^ ((v >> (8 * i)) & 0xFF)) * 0x100000001B3) & M64
    return h


class Slot:
    def __init__(self):
        self.state, self.key, self.meta, self.verified, self.pins, self.used = FREE, None, None, False, 0, 0


class CacheModel:
    """key: (hash identifier, block hash); meta: (chunk count, raw size, digest)."""

    def __init__(self, slot_count, slot_bytes):
        self.slots = [Slot() for _ in range(slot_count)]
        self.slot_bytes = (slot_bytes + 63) // 64 * 64
        self.clock = 0
        self.hits = self.inserted = self.evicted = self.bypassed = self.dropped = 0

    def lookup(self, key):
        for i, s in enumerate(self.slots):
            if s.state == VISIBLE and s.key == key:
                return i
        return NO_SLOT

    def matches(self, i, meta, need_verified):
        s = self.slots[i]
        return s.state == VISIBLE and s.meta == meta and (not need_verified or s.verified)

    def attach(self, key, meta, need_verified):
        """lookup + matches + pin, as lthip_restore_set_cache does per needed block -> the pinned slot or NO_SLOT."""
        i = self.lookup(key)
        if i == NO_SLOT or not self.matches(i, meta, need_verified):
            return NO_SLOT
        self.clock += 1
        self.slots[i].pins += 1
        self.slots[i].used = self.clock
        self.hits += 1
        return i

    def unpin(self, i):
        s = self.slots[i]
        if s.state != VISIBLE or not s.pins:
            return False
        s.pins -= 1
        return True

    def _evict(self, i):
        self.slots[i] = Slot()
        self.evicted += 1

    def reserve(self, key, meta):
        i = NO_SLOT
        if meta[1] <= self.slot_bytes:
            mine = self.lookup(key)
            if mine != NO_SLOT:
                i = NO_SLOT if self.slots[mine].pins else mine
            else:
                free = [k for k, s in enumerate(self.slots) if s.state == FREE]
                idle = sorted((s.used, k) for k, s in enumerate(self.slots) if s.state == VISIBLE and not s.pins)
                i = free[0] if free else idle[0][1] if idle else NO_SLOT
        if i == NO_SLOT:
            self.bypassed += 1
            return NO_SLOT
        if self.slots[i].state == VISIBLE:
            self._evict(i)
        s = self.slots[i]
        s.state, s.key, s.meta = RESERVED, key, meta
        return i

    def commit(self, i, verified):
        s = self.slots[i]
        if s.state != RESERVED:
            return False
        other = self.lookup(s.key)
        if other != NO_SLOT:
            if self.slots[other].pins:
                self.slots[i] = Slot()
                self.bypassed += 1
                return False
            self._evict(other)
        self.clock += 1
        s.state, s.verified, s.pins, s.used = VISIBLE, bool(verified), 0, self.clock
        self.inserted += 1
        return True

    def abort(self, i, bad):
        if self.slots[i].state != RESERVED:
            return False
        self.slots[i] = Slot()
        self.dropped += 1 if bad else 0
        return True

    def clear(self):
        if any(s.state == RESERVED or (s.state == VISIBLE and s.pins) for s in self.slots):
            return False
        self.slots = [Slot() for _ in self.slots]
        return True

    def resident(self):
        return {s.key for s in self.slots if s.state == VISIBLE}

    def lru_order(self):
        return [k for _, k in sorted((s.used, k) for k, s in enumerate(self.slots) if s.state == VISIBLE)]

    def line(self, result):
        """The state as tests/san/block_cache_driver.cpp prints it after an operation."""
        cells = []
        for k, s in enumerate(self.slots):
            if s.state == FREE:
                cells.append(f"{k}:F")
            else:
                cells.append(f"{k}:{s.state}:{s.key[0]}/{s.key[1]}:{s.meta[0]}/{s.meta[1]}/{s.meta[2]}:{s.pins}:{int(s.verified)}")
        counts = f"{self.hits} {self.inserted} {self.evicted} {self.bypassed} {self.dropped}"
        return f"{int(result)} | {' '.join(cells)} | lru {' '.join(str(k) for k in self.lru_order())} | {counts}"
