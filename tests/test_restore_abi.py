"""CPU-only checks of the restore session's interface (include/longtail_hip.h, "the restore session"): the entry points are declared
and exported by both builds, the ABI version stays 4, the gfx950 code object holds the session's kernels, lthip_restore_layout is the
plain prefix arithmetic (against numpy, on a VersionIndex built by hand), and without a GPU lthip_restore_create is refused."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

from tests.restore_util import BLK3, build_store_index, build_version_index, numpy_layout
from tests.test_abi import declared_symbols

NEW_SYMBOLS = ["lthip_restore_layout", "lthip_restore_create", "lthip_restore_destroy", "lthip_restore_needed_blocks",
               "lthip_restore_scratch_bound", "lthip_restore_blocks", "lthip_restore_finish", "lthip_restore_block_status", "lthip_seen_find"]
KERNELS = ["k_restore_resolve", "k_restore_fill", "k_restore_check_images", "k_restore_ranges", "k_restore_compare", "k_restore_scatter",
           "k_seen_find"]

# a directory, an empty file, a chunk used by two assets, an asset of one byte
NAMES = ["a/", "a/empty", "a/one", "a/two", "b/", "b/three", "b/tiny"]
CHUNK_SIZES = [4097, 15, 33, 1, 255]
ASSET_CHUNKS = [[], [], [0, 1], [2, 0], [], [4, 1, 2], [3]]


def hand_built():
    hashes = np.arange(0x1000, 0x1000 + len(CHUNK_SIZES), dtype=np.uint64)
    return build_version_index(BLK3, 32768, NAMES, ASSET_CHUNKS, hashes, CHUNK_SIZES), hashes


def layout(dll, vi, align, want_offsets=True):
    raw = np.frombuffer(vi, np.uint8)
    n, total = C.c_uint32(0xDEAD), C.c_uint64(0xDEAD)
    offs = np.full(len(NAMES), 0xDEAD, np.uint64)
    err = dll.lthip_restore_layout(raw.ctypes.data, len(raw), align, offs.ctypes.data if want_offsets else None, C.byref(n), C.byref(total))
    return err, offs, n.value, total.value


def test_entry_points_are_declared_and_exported(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_the_package_exports_the_session():
    import longtail_amd
    from longtail_amd.lib import Restore, Seen

    assert longtail_amd.Restore is Restore
    for name in ("layout", "needed_blocks", "scratch_bound", "blocks", "finish", "block_status", "close"):
        assert callable(getattr(Restore, name)), name
    assert callable(Seen.find)


def test_code_object_holds_the_restore_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        assert k in text, k


@pytest.mark.parametrize("align", [1, 16, 64])
def test_layout_is_the_prefix_arithmetic(hiplib, align):
    vi, _ = hand_built()
    sizes = [sum(CHUNK_SIZES[c] for c in cs) for cs in ASSET_CHUNKS]
    assert sizes[0] == sizes[1] == sizes[4] == 0, "a directory and an empty file are in the version"
    want, want_total = numpy_layout(sizes, align)
    err, offs, n, total = layout(hiplib.dll, vi, align)
    assert err == 0 and n == len(NAMES)
    assert (offs == want).all(), (offs, want)
    assert total == want_total
    assert all(int(o) % align == 0 for o in offs)
    err, _, n, total = layout(hiplib.dll, vi, align, want_offsets=False)  # the count and the total alone
    assert (err, n, total) == (0, len(NAMES), want_total)
    from longtail_amd.lib import Restore

    offs2, total2 = Restore.layout(vi, align, hiplib)
    assert (offs2 == want).all() and total2 == want_total


def test_layout_refusals(hiplib):
    vi, _ = hand_built()
    for align in (0, 3, 48):
        assert layout(hiplib.dll, vi, align)[0] == errno.EINVAL, align
    assert layout(hiplib.dll, vi[:-1], 16)[0] == errno.EBADF
    assert layout(hiplib.dll, vi[:20], 16)[0] == errno.EBADF
    other_version = np.frombuffer(vi, np.uint8).copy()
    other_version[0] = 1  # 0.0.1
    assert layout(hiplib.dll, other_version.tobytes(), 16)[0] == errno.EBADF
    # an asset whose chunk sizes do not sum to its size
    wrong = np.frombuffer(vi, np.uint8).copy()
    o = 24 + len(NAMES) * 16 + 2 * 8  # m_AssetSizes[2]
    wrong[o : o + 8] = np.array([4097 + 15 + 1], np.uint64).view(np.uint8)
    assert layout(hiplib.dll, wrong.tobytes(), 16)[0] == errno.EBADF


def test_create_without_a_context_is_refused(hiplib):
    vi, hashes = hand_built()
    si = build_store_index(BLK3, [(7, 0, list(range(len(CHUNK_SIZES))))], hashes, CHUNK_SIZES)
    a, b = np.frombuffer(vi, np.uint8), np.frombuffer(si, np.uint8)
    offs, total = numpy_layout([sum(CHUNK_SIZES[c] for c in cs) for cs in ASSET_CHUNKS], 16)
    h = C.c_void_p()
    err = hiplib.dll.lthip_restore_create(None, None, a.ctypes.data, len(a), b.ctypes.data, len(b), offs.ctypes.data, total, C.byref(h))
    assert err == errno.EINVAL and not h.value
    # the host-only calls refuse a null session too
    n = C.c_uint64(0)
    assert hiplib.dll.lthip_restore_needed_blocks(None, None, 0, C.byref(n)) == errno.EINVAL
    assert hiplib.dll.lthip_restore_scratch_bound(None, 0, None) == 0
    assert hiplib.dll.lthip_restore_finish(None, None) == errno.EINVAL
    assert hiplib.dll.lthip_seen_find(None, 0, None, None) == errno.EINVAL
    hiplib.dll.lthip_restore_destroy(None)
