"""CPU-only checks of the block cache's interface (include/longtail_hip.h, "a cache of decoded blocks"): the eight entry points are
declared in the header and exported by the product and the ablation build, the ABI version stays 4, the package exports BlockCache, the
gfx950 code object holds the new kernel, every entry point returns EINVAL for NULL handles without touching a device, and the result
and config structures are the size they were.  Every comparison is equality."""
import ctypes as C
import errno
import subprocess
from pathlib import Path

import numpy as np

from tests.test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["lthip_block_cache_create", "lthip_block_cache_destroy", "lthip_block_cache_contains", "lthip_block_cache_clear",
               "lthip_block_cache_stats", "lthip_restore_set_cache", "lthip_restore_from_cache", "lthip_restore_cache_stats"]
KERNELS = ["k_restore_cache_copy"]


def test_entry_points_are_declared_and_exported(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_the_code_object_holds_the_copy_kernel(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    assert not [k for k in KERNELS if k not in text]
    assert "gfx950" in text


def test_the_package_exports_the_new_names():
    import longtail_amd
    from longtail_amd import lib

    assert longtail_amd.BlockCache is lib.BlockCache
    for name in ("set_cache", "from_cache", "cache_stats"):
        assert callable(getattr(lib.Restore, name))
    for name in ("contains", "stats", "clear", "close"):
        assert callable(getattr(lib.BlockCache, name))
    assert len(lib.BLOCK_CACHE_STATS) == 10
    assert C.sizeof(lib.RestoreResult) == 8 * 14 and C.sizeof(lib.RestoreConfig) == 16, "the structures stay as they were"


def test_every_entry_point_refuses_null_handles(hiplib):
    dll = hiplib.dll
    out = np.full(10, 0xEE, np.uint64)
    hashes, held = np.arange(3, dtype=np.uint64), np.full(3, 0xEE, np.uint8)
    h = C.c_void_p(0x1234)
    assert dll.lthip_block_cache_create(None, 4, 4096, C.byref(h)) == errno.EINVAL and not h.value, "a NULL context; *out is cleared"
    assert dll.lthip_block_cache_create(None, 4, 4096, None) == errno.EINVAL
    assert dll.lthip_block_cache_create(None, 0, 4096, C.byref(h)) == errno.EINVAL
    assert dll.lthip_block_cache_create(None, 4, 0, C.byref(h)) == errno.EINVAL
    assert dll.lthip_block_cache_destroy(None) is None
    assert dll.lthip_block_cache_contains(None, 0x626C6B33, 3, hashes.ctypes.data, held.ctypes.data) == errno.EINVAL
    assert dll.lthip_block_cache_clear(None) == errno.EINVAL
    assert dll.lthip_block_cache_stats(None, out.ctypes.data) == errno.EINVAL
    assert dll.lthip_restore_set_cache(None, None) == errno.EINVAL
    assert dll.lthip_restore_from_cache(None, None) == errno.EINVAL
    assert dll.lthip_restore_cache_stats(None, out.ctypes.data) == errno.EINVAL
    assert (out == 0xEE).all() and (held == 0xEE).all(), "a refused call writes nothing"


def test_the_header_documents_the_cache_and_the_bookkeeping_is_host_code():
    header = (ROOT / "include" / "longtail_hip.h").read_text()
    assert "a cache of decoded blocks" in header and "the reference puts lib/lrublockstore in front for that" not in header
    bookkeeping = (ROOT / "longtail_amd" / "csrc" / "block_cache.h").read_text()
    assert "hip" not in bookkeeping.lower().replace("restore.hip", "").replace("longtail_hip.h", "").replace("a line of hip", "")
    assert '#include "block_cache.h"' in (ROOT / "longtail_amd" / "csrc" / "restore.hip").read_text()
