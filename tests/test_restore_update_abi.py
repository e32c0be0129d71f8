"""CPU-only checks of the update interface (include/longtail_hip.h, "updating a resident version"): the entry points are declared and
exported by both builds, the ABI version stays 4, the code object holds the new kernels, the package exports the new names, the two device
entries refuse null arguments, and lthip_version_diff gives the lists of Longtail_CreateVersionDiff -- written out by hand for versions
built by hand, and against the reference itself (oracle/_ref) on the same blobs.  Every comparison is equality."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

from tests.restore_util import BLK2, BLK3
from tests.test_abi import declared_symbols
from tests.update_util import asset_fields, build_version_index

NEW_SYMBOLS = ["lthip_restore_create_from_base", "lthip_restore_carry", "lthip_version_diff"]
KERNELS = ["k_restore_carry_bounds", "k_restore_carry_runs", "k_restore_carry_compare", "k_restore_carry_marked"]

# (name, path hash, content hash, permissions): a removed directory with a removed file inside it, an unchanged asset, one with changed
# content, one with changed permissions, one with both; the target adds two assets of equal path length and a shorter one
SOURCE = [("gone/", 50, 0, 0o755), ("gone/file.bin", 20, 1001, 0o644), ("keep.bin", 30, 1002, 0o644), ("content.bin", 10, 1003, 0o644),
          ("perm.bin", 60, 1004, 0o644), ("both.bin", 40, 1005, 0o644)]
TARGET = [("both.bin", 40, 2005, 0o755), ("new_b.bin", 70, 2001, 0o644), ("keep.bin", 30, 1002, 0o644), ("new_a.bin", 25, 2002, 0o644),
          ("perm.bin", 60, 1004, 0o600), ("content.bin", 10, 2003, 0o644), ("n.b", 90, 2004, 0o644)]
# removed: longest path first; added: shortest first, equal lengths in ascending path-hash order; modified: ascending path hash
EXPECTED = dict(source_removed=[1, 0], target_added=[6, 3, 1], source_content=[3, 5], target_content=[5, 0], source_permissions=[5, 4],
                target_permissions=[0, 4])
KEYS = ["source_removed", "target_added", "source_content", "target_content", "source_permissions", "target_permissions"]


def version(assets, hash_id=BLK3):
    """One chunk per file (its content hash names it), none for a directory."""
    files = [a for a in assets if not a[0].endswith("/")]
    chunk_of = {a[0]: k for k, a in enumerate(files)}
    return build_version_index(hash_id, 32768, [a[0] for a in assets], [[] if a[0].endswith("/") else [chunk_of[a[0]]] for a in assets],
                               [a[2] for a in files], [100 + k for k in range(len(files))], path_hashes=[a[1] for a in assets],
                               content_hashes=[a[2] for a in assets], permissions=[a[3] for a in assets])


CASES = {"hand": (SOURCE, TARGET), "empty source": ([], TARGET), "empty target": (SOURCE, []), "both empty": ([], []),
         "the same": (SOURCE, SOURCE), "reversed": (TARGET, SOURCE)}


def expected_of(case):
    src, tgt = CASES[case]
    if case == "hand":
        return EXPECTED
    none = dict.fromkeys(KEYS, [])
    if case == "empty source":  # everything is added: shortest path first, equal lengths by path hash
        return dict(none, target_added=[6, 2, 0, 4, 3, 1, 5])
    if case == "empty target":  # everything is removed: longest path first
        return dict(none, source_removed=[1, 3, 2, 5, 4, 0])
    if case == "reversed":
        return dict(source_removed=[3, 1, 6], target_added=[0, 1], source_content=[5, 0], target_content=[3, 5], source_permissions=[0, 4],
                    target_permissions=[5, 4])
    return none


def diff(dll, a, b, lists=True):
    ra, rb = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    na, nb = int(np.frombuffer(a[12:16], np.uint32)[0]), int(np.frombuffer(b[12:16], np.uint32)[0])
    counts = np.full(4, 0xDEAD, np.uint32)
    out = [np.full(max(1, n), 0xDEAD, np.uint32) for n in (na, nb, min(na, nb), min(na, nb), min(na, nb), min(na, nb))]
    err = dll.lthip_version_diff(ra.ctypes.data, len(ra), rb.ctypes.data, len(rb), *[(x.ctypes.data if lists else None) for x in out],
                                 counts.ctypes.data)
    return err, counts.tolist(), {k: x[: int(counts[c])].tolist() for k, x, c in zip(KEYS, out, (0, 1, 2, 2, 3, 3))} if lists and not err else None


def test_entry_points_are_declared_and_exported(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_code_object_holds_the_carry_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        assert k in text, k


def test_the_package_exports_the_new_names():
    import longtail_amd
    from longtail_amd.lib import Restore, RestoreResult, version_diff

    assert longtail_amd.version_diff is version_diff and longtail_amd.Restore is Restore
    assert callable(Restore.carry)
    names = [n for n, _ in RestoreResult._fields_]
    assert names[-3:] == ["base_occurrences", "base_bytes", "base_chunks_mismatched"]


def test_the_device_entries_refuse_null_arguments(hiplib):
    from longtail_amd.lib import RestoreBase

    vi = np.frombuffer(version(SOURCE), np.uint8)
    offs = np.zeros(len(SOURCE), np.uint64)
    base = RestoreBase(C.sizeof(RestoreBase), vi.ctypes.data, len(vi), offs.ctypes.data, 1 << 20)
    h = C.c_void_p(0xDEAD)
    dll = hiplib.dll
    assert dll.lthip_restore_create_from_base(None, None, C.byref(base), vi.ctypes.data, len(vi), vi.ctypes.data, len(vi), offs.ctypes.data, 0,
                                              C.byref(h)) == errno.EINVAL
    assert not h.value
    assert dll.lthip_restore_create_from_base(None, None, None, vi.ctypes.data, len(vi), vi.ctypes.data, len(vi), offs.ctypes.data, 0,
                                              C.byref(h)) == errno.EINVAL
    assert dll.lthip_restore_carry(None, None, None) == errno.EINVAL
    counts = np.zeros(4, np.uint32)
    assert dll.lthip_version_diff(None, 0, vi.ctypes.data, len(vi), None, None, None, None, None, None, counts.ctypes.data) == errno.EINVAL
    assert dll.lthip_version_diff(vi.ctypes.data, len(vi), vi.ctypes.data, len(vi), None, None, None, None, None, None, None) == errno.EINVAL


@pytest.mark.parametrize("case", list(CASES))
def test_version_diff_on_versions_built_by_hand(hiplib, case):
    src, tgt = CASES[case]
    a, b = version(src), version(tgt)
    want = expected_of(case)
    err, counts, got = diff(hiplib.dll, a, b)
    assert err == 0
    assert got == want, (got, want)
    want_counts = [len(want["source_removed"]), len(want["target_added"]), len(want["source_content"]), len(want["source_permissions"])]
    assert counts == want_counts
    err, counts, _ = diff(hiplib.dll, a, b, lists=False)  # the counts alone
    assert err == 0 and counts == want_counts
    from longtail_amd.lib import version_diff

    assert [x.tolist() for x in version_diff(a, b, hiplib)] == [want[k] for k in KEYS]


def test_the_hand_case_holds_what_it_should():
    sp, tp = {a[1]: a for a in SOURCE}, {a[1]: a for a in TARGET}
    both = set(sp) & set(tp)
    kinds = {(sp[h][2] != tp[h][2], sp[h][3] != tp[h][3]) for h in both}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    removed = [sp[h][0] for h in set(sp) - set(tp)]
    assert sorted(removed) == ["gone/", "gone/file.bin"]
    added = [tp[h][0] for h in set(tp) - set(sp)]
    assert sorted(len(n) for n in added) == [3, 9, 9]


class RefVersionDiff(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_uint32)) for n in (
        "removed_count", "added_count", "content_count", "permissions_count", "source_removed", "target_added", "source_content",
        "target_content", "source_permissions", "target_permissions")]


def ref_diff(ref, a, b):
    d = ref.dll
    d.Longtail_CreateBlake3HashAPI.restype = C.c_void_p
    d.Longtail_CreateBlake3HashAPI.argtypes = []
    d.Longtail_ReadVersionIndexFromBuffer.restype = C.c_int
    d.Longtail_ReadVersionIndexFromBuffer.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    d.Longtail_CreateVersionDiff.restype = C.c_int
    d.Longtail_CreateVersionDiff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.POINTER(RefVersionDiff))]
    d.Longtail_Free.restype = None
    d.Longtail_Free.argtypes = [C.c_void_p]
    d.Longtail_DisposeAPI.restype = None
    d.Longtail_DisposeAPI.argtypes = [C.c_void_p]
    ra, rb = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    va, vb, out = C.c_void_p(), C.c_void_p(), C.POINTER(RefVersionDiff)()
    assert d.Longtail_ReadVersionIndexFromBuffer(ra.ctypes.data, len(ra), C.byref(va)) == 0
    assert d.Longtail_ReadVersionIndexFromBuffer(rb.ctypes.data, len(rb), C.byref(vb)) == 0
    api = d.Longtail_CreateBlake3HashAPI()
    try:
        assert d.Longtail_CreateVersionDiff(api, va, vb, C.byref(out)) == 0
        v = out.contents
        n = [v.removed_count[0], v.added_count[0], v.content_count[0], v.content_count[0], v.permissions_count[0], v.permissions_count[0]]
        lists = [v.source_removed, v.target_added, v.source_content, v.target_content, v.source_permissions, v.target_permissions]
        return {k: [int(p[i]) for i in range(c)] for k, p, c in zip(KEYS, lists, n)}
    finally:
        if out:
            d.Longtail_Free(out)
        d.Longtail_DisposeAPI(api)
        d.Longtail_Free(va)
        d.Longtail_Free(vb)


@pytest.mark.parametrize("case", list(CASES))
def test_version_diff_against_the_reference(hiplib, ref, case):
    src, tgt = CASES[case]
    a, b = version(src), version(tgt)
    want = ref_diff(ref, a, b)
    err, _, got = diff(hiplib.dll, a, b)
    assert err == 0
    for k in KEYS[2:]:
        assert got[k] == want[k], k  # the four modified lists: identical
    for k, blob, order in (("source_removed", a, -1), ("target_added", b, 1)):
        assert len(got[k]) == len(want[k])
        lens = [len(n) for n in asset_fields(blob)["names"]]
        for lists in (got[k], want[k]):
            seq = [lens[i] * order for i in lists]
            assert seq == sorted(seq), (k, "path lengths monotone")
        for n in set(lens):
            assert {i for i in got[k] if lens[i] == n} == {i for i in want[k] if lens[i] == n}, (k, n)


def test_version_diff_refusals(hiplib):
    a, b = version(SOURCE), version(TARGET)
    assert diff(hiplib.dll, a[:-1], b)[0] == errno.EBADF  # truncated: the last path loses its terminator
    assert diff(hiplib.dll, a, b[:40])[0] == errno.EBADF
    twice = [list(x) for x in TARGET]
    twice[3][1] = twice[1][1]  # two assets of one version with the same path hash
    assert diff(hiplib.dll, a, version([tuple(x) for x in twice]))[0] == errno.EBADF
    assert diff(hiplib.dll, version([tuple(x) for x in twice]), a)[0] == errno.EBADF
    assert diff(hiplib.dll, a, version(TARGET, BLK2))[0] == errno.EINVAL  # differing hash identifiers
