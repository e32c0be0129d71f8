"""CPU-only checks of the window-restore interface (include/longtail_hip.h, "byte windows of assets"): the three entry points are declared
and exported by both builds, lthip_restore_window is 32 bytes in the header and in the ctypes mirror, the package exports the new names,
lthip_restore_asset_sizes agrees with the blob, lthip_restore_rank_windows agrees with a dozen lines of numpy (the tree of the GPU
rank-share test and the size list of BASELINE configs[4]: four assets of 16 GiB, target 32768, 8 ranks -- host arithmetic, no memory of
that size), and lthip_restore_create_windows is refused without a context like lthip_restore_create.  Every comparison is equality."""
import ctypes as C
import errno
import re
from pathlib import Path

import numpy as np
import pytest

from longtail_amd.dist import JobPartition
from tests.restore_util import BLK3, build_store_index, build_version_index, parse_version_index
from tests.restore_windows_util import SHARE_NAMES, SHARE_SIZES, model_rank_windows, share_tree
from tests.test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["lthip_restore_create_windows", "lthip_restore_asset_sizes", "lthip_restore_rank_windows"]
POLICIES = ["range", "lpt", "mod"]


def share_version():
    files, chunks, asset_chunks, lens, blocks = share_tree()
    hashes = np.arange(500, 500 + len(chunks), dtype=np.uint64)
    return build_version_index(BLK3, 1, SHARE_NAMES, asset_chunks, hashes, lens), build_store_index(BLK3, [(1, 0, blocks[0])], hashes, lens)


def test_entry_points_are_declared_and_exported(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_the_window_is_32_bytes_here_and_in_the_header():
    from longtail_amd.lib import RESTORE_WINDOW_DTYPE, RestoreWindow

    assert C.sizeof(RestoreWindow) == 32 == RESTORE_WINDOW_DTYPE.itemsize
    assert [(n, getattr(RestoreWindow, n).offset) for n, _ in RestoreWindow._fields_] == [("asset", 0), ("reserved", 4), ("offset", 8),
                                                                                         ("length", 16), ("dst", 24)]
    assert [RESTORE_WINDOW_DTYPE.fields[n][1] for n, _ in RestoreWindow._fields_] == [0, 4, 8, 16, 24]
    header = (ROOT / "include" / "longtail_hip.h").read_text()
    assert re.search(r"static_assert\(sizeof\(lthip_restore_window\) == 32", header)
    assert "restore_windows.h" in (ROOT / "longtail_amd" / "csrc" / "restore.hip").read_text()


def test_the_package_exports_the_new_names():
    import longtail_amd
    from longtail_amd import lib

    assert longtail_amd.RestoreWindow is lib.RestoreWindow
    assert longtail_amd.restore_asset_sizes is lib.restore_asset_sizes and longtail_amd.restore_rank_windows is lib.restore_rank_windows
    with pytest.raises(ValueError):
        lib.Restore(None, b"", b"", [0], 0, windows=[(0, 0, 0, 0)])  # both asset_offsets and windows
    with pytest.raises(ValueError):
        lib.Restore(None, b"", b"", None, 0, windows=[(0, 0, 0, 0)], base=(b"", [], 0))  # windows with a base


def test_asset_sizes_are_the_blobs(hiplib):
    from longtail_amd.lib import LongtailHipError, restore_asset_sizes

    vi, _ = share_version()
    sizes, target = restore_asset_sizes(vi, hiplib)
    assert sizes.tolist() == parse_version_index(vi)["sizes"].tolist() == SHARE_SIZES and target == 1
    raw = np.frombuffer(vi, np.uint8)
    n, t = C.c_uint32(77), C.c_uint32(77)
    assert hiplib.dll.lthip_restore_asset_sizes(raw.ctypes.data, len(raw), None, C.byref(n), C.byref(t)) == 0 and (n.value, t.value) == (7, 1)
    assert hiplib.dll.lthip_restore_asset_sizes(raw.ctypes.data, len(raw), None, None, None) == 0
    assert hiplib.dll.lthip_restore_asset_sizes(None, len(raw), None, C.byref(n), C.byref(t)) == errno.EINVAL
    for cut in (1, 23, len(vi) - 1):
        with pytest.raises(LongtailHipError) as e:
            restore_asset_sizes(vi[:cut], hiplib)
        assert e.value.code == errno.EBADF


def check_rank_windows(hiplib, sizes, target, world, policy, align):
    """Every rank's table is the model's; together the ranks' windows cover every byte of every asset exactly once."""
    from longtail_amd.lib import restore_rank_windows

    part = JobPartition(sizes, target, world, policy, lib=hiplib)
    spans = []
    for rank in range(world):
        rows, total = restore_rank_windows(part.job_asset, part.job_offset, part.job_size, part.job_rank, rank, align, hiplib)
        want, want_total = model_rank_windows(part.job_asset, part.job_offset, part.job_size, part.job_rank, rank, align)
        assert [tuple(int(x) for x in r) for r in rows] == want and total == want_total
        assert all(int(r[3]) % align == 0 for r in rows)
        assert sum(int(r[2]) for r in rows) == int(part.rank_bytes[rank])
        ends = [(int(r[3]), int(r[3]) + int(r[2])) for r in rows]
        assert all(p[1] <= q[0] for p, q in zip(ends, ends[1:])) and (not ends or ends[-1][1] == total)
        spans += [(int(r[0]), int(r[1]), int(r[1]) + int(r[2])) for r in rows]
    spans.sort()
    for a, size in enumerate(sizes):
        mine = [(lo, hi) for x, lo, hi in spans if x == a]
        assert ([lo for lo, _ in mine] + [size])[0] == (0 if size else size)
        assert all(p[1] == q[0] for p, q in zip(mine, mine[1:])) and (mine[-1][1] if mine else 0) == size
    return part


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("world", [2, 3])
def test_rank_windows_of_the_small_tree_are_the_models(hiplib, world, policy, align):
    part = check_rank_windows(hiplib, SHARE_SIZES, 1, world, policy, align)
    assert part.job_count == sum(1 + s // 1024 for s in SHARE_SIZES)


@pytest.mark.parametrize("policy", POLICIES)
def test_rank_windows_of_four_16_gib_assets_over_eight_ranks(hiplib, policy):
    from longtail_amd.lib import restore_rank_windows

    sizes = [16 << 30] * 4
    part = check_rank_windows(hiplib, sizes, 32768, 8, policy, 4096)
    if policy == "range":  # every asset straddles two ranks: each rank holds half an asset, in ONE window
        for rank in range(8):
            rows, total = restore_rank_windows(part.job_asset, part.job_offset, part.job_size, part.job_rank, rank, 4096, hiplib)
            assert [tuple(int(x) for x in r) for r in rows] == [(rank // 2, (rank % 2) * (8 << 30), 8 << 30, 0)] and total == 8 << 30


def test_rank_windows_counts_and_refusals(hiplib):
    part = JobPartition(SHARE_SIZES, 1, 2, "mod", lib=hiplib)
    want, want_total = model_rank_windows(part.job_asset, part.job_offset, part.job_size, part.job_rank, 1, 16)
    assert len(want) >= 3
    args = (part.job_count, part.job_asset.ctypes.data, part.job_offset.ctypes.data, part.job_size.ctypes.data, part.job_rank.ctypes.data, 1)
    n, total = C.c_uint64(0), C.c_uint64(0)
    table = np.full(4 * len(want), 0xEE, np.uint64)
    call = hiplib.dll.lthip_restore_rank_windows
    assert call(*args, 16, None, 0, C.byref(n), C.byref(total)) == 0 and (n.value, total.value) == (len(want), want_total)
    assert call(*args, 16, table.ctypes.data, len(want) - 1, C.byref(n), None) == errno.ENOMEM and n.value == len(want)
    assert (table == 0xEE).all(), "too small a capacity: the count only"
    assert call(*args, 16, table.ctypes.data, len(want), C.byref(n), C.byref(total)) == 0
    assert [(int(r[0]) & 0xFFFFFFFF, int(r[0]) >> 32, int(r[1]), int(r[2]), int(r[3])) for r in table.reshape(-1, 4)] == \
        [(a, 0, o, k, d) for a, o, k, d in want]
    for align in (0, 3, 24):
        assert call(*args, align, None, 0, C.byref(n), C.byref(total)) == errno.EINVAL
    assert call(*args, 16, None, 0, None, C.byref(total)) == errno.EINVAL
    assert call(part.job_count, None, *args[2:], 16, None, 0, C.byref(n), None) == errno.EINVAL
    assert call(0, None, None, None, None, 0, 1, None, 0, C.byref(n), C.byref(total)) == 0 and (n.value, total.value) == (0, 0)
    # a rank without jobs, and a rank that does not exist: no windows
    assert call(*args[:5], 5, 16, None, 0, C.byref(n), C.byref(total)) == 0 and (n.value, total.value) == (0, 0)


def test_create_windows_is_refused_without_a_context_like_create(hiplib):
    vi, si = share_version()
    a, b = np.frombuffer(vi, np.uint8), np.frombuffer(si, np.uint8)
    offs = np.zeros(len(SHARE_SIZES), np.uint64)
    table = np.zeros(4, np.uint64)
    h = C.c_void_p(0x1234)
    dll = hiplib.dll
    want = dll.lthip_restore_create(None, None, a.ctypes.data, len(a), b.ctypes.data, len(b), offs.ctypes.data, 1 << 20, C.byref(h))
    assert want == errno.EINVAL
    h = C.c_void_p(0x1234)
    assert dll.lthip_restore_create_windows(None, None, a.ctypes.data, len(a), b.ctypes.data, len(b), 1, table.ctypes.data, 1 << 20, C.byref(h)) == want
    assert dll.lthip_restore_create_windows(None, None, a.ctypes.data, len(a), b.ctypes.data, len(b), 1, table.ctypes.data, 1 << 20, None) == want
