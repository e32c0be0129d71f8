"""CPU-only checks of the store index operations (include/longtail_hip.h, "store index operations"; longtail_amd/csrc/store_index_ops.h):
lthip_store_index_prune and lthip_store_index_merge against the reference (Longtail_PruneStoreIndex / Longtail_MergeStoreIndex followed
by Longtail_WriteStoreIndexToBuffer through ctypes on oracle/_ref, skipped where it is not built) and against the reference's results
as recorded in tests/golden/store_index_ops_ref.npz, which every machine has; lthip_version_chunk_hashes against a Python reading of the
VersionIndex.  Blobs and outputs lie at odd addresses throughout.  Every comparison is equality."""
import ctypes as C
import errno

import numpy as np
import pytest

from longtail_amd.lib import LongtailHipError, store_index_merge, store_index_prune, version_chunk_hashes
from tests._libs import have_ref
from tests.restore_util import BLK2, BLK3, build_version_index, parse_store_index, parse_version_index
from tests.store_index_ops_util import A, B, EMPTY, HASHES, LZ4, MERGES, NO_CHUNKS, ONES, OTHER_HASH, PRUNES, SIZES, TWICE, TWICE_REMOTE, RefOps, bare_head, golden, index
from tests.test_abi import declared_symbols

NEW_SYMBOLS = ["lthip_store_index_prune", "lthip_store_index_merge", "lthip_version_chunk_hashes"]
FILL = 0xEE


def odd(blob: bytes):
    """The blob's bytes at an odd address -> (the array that owns them, the address)."""
    own = np.zeros(len(blob) + 1, np.uint8)
    own[1:] = np.frombuffer(blob, np.uint8)
    assert (own.ctypes.data + 1) % 2 == 1
    return own, own.ctypes.data + 1


def call_at_odd_addresses(fn, *blobs_and_args):
    """fn(blob pointers and sizes..., out, capacity, &size) with every blob and the output at an odd address: first for the size, then one
    byte short (nothing written), then for the bytes.  -> the bytes, or the errno."""
    keep, args = [], []
    for a in blobs_and_args:
        if isinstance(a, bytes):
            own, p = odd(a)
            keep.append(own)
            args += [p, len(a)]
        else:
            args.append(a)
    n = C.c_size_t(0xEEEE)
    err = fn(*args, None, 0, C.byref(n))
    if err != errno.ENOMEM:
        assert err != 0 and n.value == 0xEEEE, "a refused call leaves the size alone"
        return err
    need = n.value
    out = np.full(need + 2, FILL, np.uint8)
    n = C.c_size_t(0)
    assert fn(*args, out.ctypes.data + 1, need - 1, C.byref(n)) == errno.ENOMEM and n.value == need, "ENOMEM with the size set"
    assert (out == FILL).all(), "a refused call writes nothing"
    assert fn(*args, out.ctypes.data + 1, need, C.byref(n)) == 0 and n.value == need
    assert out[0] == FILL and out[-1] == FILL
    return out[1:-1].tobytes()


def ours_merge(hiplib, local, remote):
    return call_at_odd_addresses(hiplib.dll.lthip_store_index_merge, local, remote)


def ours_prune(hiplib, si, keep):
    k = np.ascontiguousarray(keep, np.uint64)
    return call_at_odd_addresses(hiplib.dll.lthip_store_index_prune, si, C.c_uint32(len(k)), C.c_void_p(k.ctypes.data if len(k) else None))


def test_entry_points_are_declared_and_exported_and_the_abi_version_stays(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_the_package_exports_the_new_names():
    import longtail_amd
    from longtail_amd import lib

    for name in ("store_index_prune", "store_index_merge", "version_chunk_hashes"):
        assert getattr(longtail_amd, name) is getattr(lib, name)


@pytest.mark.parametrize("name", list(MERGES))
def test_merge_is_the_recorded_reference_result(hiplib, name):
    want = golden()[("merge", name)]
    assert ours_merge(hiplib, *MERGES[name]) == want
    if isinstance(want, bytes):
        assert store_index_merge(*MERGES[name]) == want


@pytest.mark.parametrize("name", list(PRUNES))
def test_prune_is_the_recorded_reference_result(hiplib, name):
    want = golden()[("prune", name)]
    assert ours_prune(hiplib, *PRUNES[name]) == want
    assert store_index_prune(*PRUNES[name]) == want


def test_the_recorded_results_are_what_the_rules_say(hiplib):
    """The golden file read against the rules in words, so that a wrong recording cannot pass as the reference."""
    g = golden()
    assert set(g) == {("merge", n) for n in MERGES} | {("prune", n) for n in PRUNES}
    assert g[("merge", "empty + empty")] == g[("merge", "a kept-nothing local + empty")] == bare_head(0), "identifier 0 when both sides are empty"
    assert g[("merge", "empty local")] == A and g[("merge", "empty remote")] == A and g[("merge", "with itself")] == A
    assert g[("merge", "conflicting identifiers")] == errno.EINVAL
    assert g[("merge", "blocks without chunks carry identifier 0 and conflict")] == errno.EINVAL
    assert parse_store_index(g[("merge", "a local without blocks does not conflict")])["hash_id"] == BLK2
    assert g[("merge", "a remote without blocks does not conflict")] == OTHER_HASH
    ab = parse_store_index(g[("merge", "disjoint but one block with another tag")])
    assert [int(h) for h in ab["block_hashes"]] == [0xA1, 0xA2, 0xA3, 0, ONES, 0xB1, 0xB2], "local first, then what local lacks"
    assert [int(t) for t in ab["block_tags"][[1, 4]]] == [LZ4, LZ4] and int(ab["block_counts"][1]) == 1, "local wins a block both sides hold"
    ba = parse_store_index(g[("merge", "the other way round")])
    assert [int(h) for h in ba["block_hashes"]] == [0xB1, 0xA2, 0xB2, ONES, 0xA1, 0xA3, 0]
    assert [int(t) for t in ba["block_tags"][[1, 3]]] == [0, 0] and int(ba["block_counts"][1]) == 3
    tw = parse_store_index(g[("merge", "a block hash twice in local")])
    assert [int(h) for h in tw["block_hashes"]] == [0xD1, 0xD2, 0xD3, 0xD4] and [int(c) for c in tw["block_counts"]] == [2, 1, 1, 2]
    assert [int(t) for t in tw["block_tags"]] == [0, LZ4, 0, 0], "the first occurrence wins the tag and the chunk list"
    assert (tw["chunk_hashes"] == HASHES[[0, 1, 2, 6, 8, 9]]).all() and (tw["chunk_sizes"] == SIZES[[0, 1, 2, 6, 8, 9]]).all()
    assert [int(o) for o in tw["block_offsets"]] == [0, 2, 3, 4]
    none = g[("prune", "keep nothing")]
    assert none == bare_head(BLK3), "a prune keeps the identifier"
    assert g[("prune", "keep everything")] == A and g[("prune", "an empty index")] == EMPTY
    rep = parse_store_index(g[("prune", "repeats, unknown hashes, another order")])
    assert [int(h) for h in rep["block_hashes"]] == [0xA1, 0xA3, ONES] and [int(o) for o in rep["block_offsets"]] == [0, 3, 7]
    kept_twice = parse_store_index(g[("prune", "a block hash that stands twice is kept twice")])
    assert [int(h) for h in kept_twice["block_hashes"]] == [0xD1, 0xD1, 0xD3] and [int(c) for c in kept_twice["block_counts"]] == [2, 3, 1]


def test_merge_of_a_prune(hiplib):
    """The two together: the blocks a caller keeps, then the blocks it adds."""
    kept = store_index_prune(A, [0xA3, 0xA1])
    merged = parse_store_index(store_index_merge(kept, B))
    assert [int(h) for h in merged["block_hashes"]] == [0xA1, 0xA3, 0xB1, 0xA2, 0xB2, ONES]
    assert store_index_merge(store_index_prune(A, []), EMPTY) == bare_head(0)


def test_truncated_and_malformed_blobs_are_ebadf(hiplib):
    for blob in (A, TWICE, NO_CHUNKS):
        for n in range(len(blob)):
            assert ours_prune(hiplib, blob[:n] or b"", [0xA1]) == errno.EBADF, n
            assert ours_merge(hiplib, blob[:n], B) == errno.EBADF and ours_merge(hiplib, B, blob[:n]) == errno.EBADF, n

    def word(blob, at, value):
        b = bytearray(blob)
        b[at : at + 4] = int(value).to_bytes(4, "little")
        return bytes(b)

    nb, m = 5, 11
    cases = {"another version": word(A, 0, 2), "a hash identifier that names no hash": word(A, 4, 0x12345678), "block count": word(A, 8, 0x20000000),
             "chunk count": word(A, 12, 0xAAAAAAAB), "a chunk run past the list": word(A, 16 + 8 * nb + 8 * m + 4 * (nb - 1), m - 1),
             "identifier 0 with chunks": word(A, 4, 0)}
    for what, bad in cases.items():
        assert ours_prune(hiplib, bad, [0xA1]) == errno.EBADF, what
        assert ours_merge(hiplib, bad, EMPTY) == errno.EBADF and ours_merge(hiplib, EMPTY, bad) == errno.EBADF, what
    with pytest.raises(LongtailHipError) as e:
        store_index_merge(A[:-1], B)
    assert e.value.code == errno.EBADF


def test_null_arguments_are_einval_and_write_nothing(hiplib):
    dll = hiplib.dll
    own, p = odd(A)
    n = C.c_size_t(0xEE)
    out = np.full(64, FILL, np.uint8)
    assert dll.lthip_store_index_prune(None, 0, 0, None, out.ctypes.data, 64, C.byref(n)) == errno.EINVAL
    assert dll.lthip_store_index_prune(p, len(A), 2, None, out.ctypes.data, 64, C.byref(n)) == errno.EINVAL, "a keep count without a list"
    assert dll.lthip_store_index_prune(p, len(A), 0, None, out.ctypes.data, 64, None) == errno.EINVAL
    assert dll.lthip_store_index_merge(None, 0, p, len(A), out.ctypes.data, 64, C.byref(n)) == errno.EINVAL
    assert dll.lthip_store_index_merge(p, len(A), None, 0, out.ctypes.data, 64, C.byref(n)) == errno.EINVAL
    assert dll.lthip_store_index_merge(p, len(A), p, len(A), out.ctypes.data, 64, None) == errno.EINVAL
    assert dll.lthip_version_chunk_hashes(None, 0, None, 0, C.byref(n)) == errno.EINVAL
    assert dll.lthip_version_chunk_hashes(p, len(A), None, 0, None) == errno.EINVAL
    assert n.value == 0xEE and (out == FILL).all()


def test_version_chunk_hashes_is_the_version_indexes_list(hiplib):
    names = ["a.bin", "dir/", "dir/b.bin", "empty"]
    vi = build_version_index(BLK3, 4096, names, [[0, 1, 2, 1], [], [3, 0, 4], []], HASHES[:5], SIZES[:5])
    want = parse_version_index(vi)["chunk_hashes"]
    assert (version_chunk_hashes(vi) == want).all() and len(want) == 5
    own, p = odd(vi)
    n = C.c_uint64(0xEE)
    assert hiplib.dll.lthip_version_chunk_hashes(p, len(vi), None, 0, C.byref(n)) == errno.ENOMEM and n.value == 5, "the count alone"
    out = np.full(6, FILL, np.uint64)
    assert hiplib.dll.lthip_version_chunk_hashes(p, len(vi), out.ctypes.data, 4, C.byref(n)) == errno.ENOMEM and n.value == 5
    assert (out == FILL).all(), "a refused call writes nothing"
    assert hiplib.dll.lthip_version_chunk_hashes(p, len(vi), out.ctypes.data, 5, C.byref(n)) == 0 and (out[:5] == want).all() and out[5] == FILL
    for k in range(len(vi)):
        own, p = odd(vi[:k])
        n = C.c_uint64(0xEE)
        assert hiplib.dll.lthip_version_chunk_hashes(p, k, None, 0, C.byref(n)) == errno.EBADF and n.value == 0xEE, k
    none = build_version_index(BLK3, 4096, ["dir/"], [[]], HASHES[:0], SIZES[:0])
    assert len(version_chunk_hashes(none)) == 0
    own, p = odd(none)
    assert hiplib.dll.lthip_version_chunk_hashes(p, len(none), None, 0, C.byref(n)) == 0 and n.value == 0, "a version without chunks"


# ---- against the reference ----

needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/liblongtail_ref.so not built (needs /root/reference at build time)")


@needs_ref
@pytest.mark.parametrize("name", list(MERGES))
def test_merge_equals_the_reference(hiplib, ref, name):
    theirs = RefOps(ref).merge(*MERGES[name])
    assert ours_merge(hiplib, *MERGES[name]) == theirs
    assert golden()[("merge", name)] == theirs, "the recorded result is out of date: tools/gen_store_index_ops_golden.py"


@needs_ref
@pytest.mark.parametrize("name", list(PRUNES))
def test_prune_equals_the_reference(hiplib, ref, name):
    theirs = RefOps(ref).prune(*PRUNES[name])
    assert ours_prune(hiplib, *PRUNES[name]) == theirs
    assert golden()[("prune", name)] == theirs, "the recorded result is out of date: tools/gen_store_index_ops_golden.py"


@needs_ref
def test_random_indexes_equal_the_reference(hiplib, ref):
    """Seeded random pairs: block hashes from a pool of 12 (so that repeats inside and across the sides are common), 0 to 4 chunks a
    block, four tags; every pair is merged both ways and each side pruned by a random keep list."""
    r = RefOps(ref)
    rng = np.random.default_rng(31)
    pool = [0, ONES] + [int(x) for x in rng.integers(1, 2**63, 10)]
    tags = [0, LZ4, 0x7A746431, 0x62746C30]

    def random_index():
        blocks, at = [], 0
        for _ in range(int(rng.integers(0, 9))):
            n = int(rng.integers(0, 5))
            blocks.append((pool[int(rng.integers(0, len(pool)))], tags[int(rng.integers(0, 4))], [(at + k) % 40 for k in range(n)]))
            at += n
        return index(BLK3, blocks)

    for _ in range(40):
        a, b = random_index(), random_index()
        for x, y in ((a, b), (b, a)):
            assert ours_merge(hiplib, x, y) == r.merge(x, y)
        keep = [pool[int(k)] for k in rng.integers(0, len(pool), int(rng.integers(0, 8)))]
        assert ours_prune(hiplib, a, keep) == r.prune(a, keep)
