"""Helpers of the store-index-operation tests: the cases (hand-built StoreIndexes, tests/restore_util.py), the reference's two functions
through ctypes (Longtail_PruneStoreIndex / Longtail_MergeStoreIndex of oracle/_ref/liblongtail_ref.so, each followed by
Longtail_WriteStoreIndexToBuffer) and the results it gave, recorded in tests/golden/store_index_ops_ref.npz
(tools/gen_store_index_ops_golden.py) for machines without it."""
import ctypes as C

import numpy as np

from tests._libs import GOLDEN
from tests.restore_util import BLK2, BLK3, STORE_INDEX_VERSION, build_store_index

LZ4, ZSTD2 = 0x6C7A3432, 0x7A746432
GOLDEN_FILE = GOLDEN / "store_index_ops_ref.npz"
ONES = 0xFFFFFFFFFFFFFFFF

HASHES = np.arange(5000, 5040, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
SIZES = (np.arange(40, dtype=np.uint32) * 37) % 251 + 1


def index(hash_id, blocks):
    return build_store_index(hash_id, blocks, HASHES, SIZES)


def bare_head(hash_id):
    """A StoreIndex without blocks that still names a hash type: what a prune that keeps nothing leaves."""
    return np.array([STORE_INDEX_VERSION, hash_id, 0, 0], np.uint32).tobytes()


EMPTY = index(BLK3, [])
A = index(BLK3, [(0xA1, 0, [0, 1, 2]), (0xA2, LZ4, [3]), (0xA3, ZSTD2, [4, 5, 6, 7]), (0, 0, [8]), (ONES, LZ4, [9, 10])])
B = index(BLK3, [(0xB1, LZ4, [11, 12]), (0xA2, 0, [13, 14, 15]), (0xB2, 0, []), (ONES, 0, [16])])
TWICE = index(BLK3, [(0xD1, 0, [0, 1]), (0xD2, LZ4, [2]), (0xD1, ZSTD2, [3, 4, 5]), (0xD3, 0, [6])])
TWICE_REMOTE = index(BLK3, [(0xD1, LZ4, [7]), (0xD4, 0, [8, 9]), (0xD4, LZ4, [10]), (0xD2, 0, [11])])
OTHER_HASH = index(BLK2, [(0xC1, 0, [20, 21]), (0xC2, LZ4, [22])])
NO_CHUNKS = index(BLK3, [(0xE1, 0, []), (0xE2, LZ4, [])])  # blocks, but no chunk: the identifier is 0

MERGES = {
    "empty + empty": (EMPTY, EMPTY),
    "a kept-nothing local + empty": (bare_head(BLK3), EMPTY),
    "empty local": (EMPTY, A),
    "empty remote": (A, EMPTY),
    "disjoint but one block with another tag": (A, B),
    "the other way round": (B, A),
    "with itself": (A, A),
    "a block hash twice in local": (TWICE, TWICE_REMOTE),
    "a block hash twice in remote": (TWICE_REMOTE, TWICE),
    "conflicting identifiers": (A, OTHER_HASH),
    "a local without blocks does not conflict": (bare_head(BLK3), OTHER_HASH),
    "a remote without blocks does not conflict": (OTHER_HASH, bare_head(BLK3)),
    "blocks without chunks carry identifier 0 and conflict": (NO_CHUNKS, A),
    "blocks without chunks alone": (NO_CHUNKS, EMPTY),
}

PRUNES = {
    "keep nothing": (A, []),
    "keep everything": (A, [0xA1, 0xA2, 0xA3, 0, ONES]),
    "repeats, unknown hashes, another order": (A, [ONES, 0xA3, 0x77, 0xA3, ONES, 0xA1, 0x78, 0xA1]),
    "hash 0 alone": (A, [0]),
    "a block hash that stands twice is kept twice": (TWICE, [0xD1, 0xD3]),
    "the other blocks of it": (TWICE, [0xD2]),
    "an empty index": (EMPTY, [1, 2]),
    "blocks without chunks": (NO_CHUNKS, [0xE2]),
    "another hash type": (OTHER_HASH, [0xC2]),
}


class RefOps:
    """-> the serialized result of the reference, or its errno (an int)."""

    def __init__(self, ref):
        d = self.d = ref.dll
        p = C.c_void_p
        for name, res, args in (("Longtail_ReadStoreIndexFromBuffer", C.c_int, [p, C.c_size_t, C.POINTER(p)]),
                                ("Longtail_WriteStoreIndexToBuffer", C.c_int, [p, C.POINTER(p), C.POINTER(C.c_size_t)]),
                                ("Longtail_PruneStoreIndex", C.c_int, [p, C.c_uint32, p, C.POINTER(p)]),
                                ("Longtail_MergeStoreIndex", C.c_int, [p, p, C.POINTER(p)]), ("Longtail_Free", None, [p])):
            f = getattr(d, name)
            f.restype, f.argtypes = res, args

    def _read(self, blob: bytes):
        raw, out = np.frombuffer(blob, np.uint8).copy(), C.c_void_p()
        err = self.d.Longtail_ReadStoreIndexFromBuffer(raw.ctypes.data, len(raw), C.byref(out))
        assert err == 0, err
        return out

    def _write_and_free(self, err, result, inputs):
        try:
            if err:
                return int(err)
            buf, size = C.c_void_p(), C.c_size_t(0)
            assert self.d.Longtail_WriteStoreIndexToBuffer(result, C.byref(buf), C.byref(size)) == 0
            out = C.string_at(buf.value, size.value)
            self.d.Longtail_Free(buf)
            return out
        finally:
            for p in (result, *inputs):
                if p.value:
                    self.d.Longtail_Free(p)

    def prune(self, store_index: bytes, keep):
        s, out = self._read(store_index), C.c_void_p()
        k = np.ascontiguousarray(keep, np.uint64)
        err = self.d.Longtail_PruneStoreIndex(s, len(k), k.ctypes.data if len(k) else None, C.byref(out))
        return self._write_and_free(err, out, [s])

    def merge(self, local: bytes, remote: bytes):
        a, b, out = self._read(local), self._read(remote), C.c_void_p()
        err = self.d.Longtail_MergeStoreIndex(a, b, C.byref(out))
        return self._write_and_free(err, out, [a, b])


def golden():
    """{("merge" | "prune", case name): bytes or errno} as the reference gave it when the file was recorded."""
    g = np.load(GOLDEN_FILE)
    out = {}
    for key in g.files:
        op, kind, name = key.split("/", 2)
        out[(op, name)] = g[key].tobytes() if kind == "out" else int(g[key])
    return out
