"""CPU-only checks of the repack session's interface (include/longtail_hip.h, "the repack session"): the entry points are declared and
exported by both builds, the ABI version stays 4, the structs of the binding are as large as the header's (a C compiler says so), the
gfx950 code object holds the plan's kernels, the header prints the safety contract, and without a session every call refuses."""
import ctypes as C
import errno
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["lthip_repack_create", "lthip_repack_destroy", "lthip_repack_plan_info", "lthip_repack_kept_blocks", "lthip_repack_dropped_blocks",
               "lthip_repack_source_blocks", "lthip_repack_kept_index", "lthip_repack_scratch_bound", "lthip_repack_blocks", "lthip_repack_write",
               "lthip_repack_finish", "lthip_repack_images", "lthip_repack_store_index", "lthip_repack_block_status"]
KERNELS = ["k_repack_resolve", "k_repack_compact", "k_repack_dest"]


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
    from longtail_amd.lib import Repack

    assert longtail_amd.Repack is Repack
    for name in ("info", "kept_blocks", "dropped_blocks", "source_blocks", "kept_index", "scratch_bound", "blocks", "write", "finish", "images",
                 "store_index", "block_status", "close"):
        assert callable(getattr(Repack, name)), name


def test_struct_sizes_are_the_headers():
    from longtail_amd.lib import RepackConfig, RepackInfo, RepackResult

    assert (C.sizeof(RepackConfig), C.sizeof(RepackInfo), C.sizeof(RepackResult)) == (24, 14 * 8, 8 * 8)
    assert RepackConfig.max_chunks_per_block.offset == 16 and RepackConfig.verify.offset == 20
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "longtail_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", '
            "sizeof(lthip_repack_config), sizeof(lthip_repack_info), sizeof(lthip_repack_result), offsetof(lthip_repack_config, verify), "
            "offsetof(lthip_repack_info, store_index_size));return 0;}\n")
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "sizes"
        build = subprocess.run([cc, "-std=c99", "-I", str(ROOT / "include"), "-x", "c", "-", "-o", str(exe)], input=prog, capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(x) for x in got] == [C.sizeof(RepackConfig), C.sizeof(RepackInfo), C.sizeof(RepackResult), RepackConfig.verify.offset,
                                     RepackInfo.store_index_size.offset]


def test_code_object_holds_the_plan_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        assert k in text, k


def test_the_header_prints_the_safety_contract():
    text = " ".join((ROOT / "include" / "longtail_hip.h").read_text().split())
    assert "delete dropped blocks only after lthip_repack_finish returned 0 and the new images are stored" in text


def test_calls_without_a_session_or_context_are_refused(hiplib):
    from longtail_amd.lib import RepackConfig, RepackInfo

    d = hiplib.dll
    si = np.array([1 << 24, 0, 0, 0], np.uint32)
    cfg = RepackConfig(C.sizeof(RepackConfig), 50, 1 << 20, 1024, 1)
    h = C.c_void_p(0xDEAD)
    assert d.lthip_repack_create(None, C.byref(cfg), si.ctypes.data, si.nbytes, 0, None, C.byref(h)) == errno.EINVAL and not h.value
    n, z = C.c_uint64(0), C.c_size_t(0)
    info = RepackInfo()
    info.struct_size = C.sizeof(RepackInfo)
    assert d.lthip_repack_plan_info(None, C.byref(info)) == errno.EINVAL
    for name in ("kept", "dropped", "source"):
        assert getattr(d, f"lthip_repack_{name}_blocks")(None, None, 0, C.byref(n)) == errno.EINVAL
    assert d.lthip_repack_kept_index(None, None, 0, C.byref(z)) == errno.EINVAL
    assert d.lthip_repack_scratch_bound(None, 0, None) == 0
    assert d.lthip_repack_blocks(None, 0, None, None, None, None, None, 0, None) == errno.EINVAL
    assert d.lthip_repack_write(None, None, 0) == errno.EINVAL
    assert d.lthip_repack_finish(None, None, 0, C.byref(z), None) == errno.EINVAL
    assert d.lthip_repack_images(None, C.byref(n), None, None) == errno.EINVAL
    assert d.lthip_repack_store_index(None, None, 0, C.byref(z)) == errno.EINVAL
    assert d.lthip_repack_block_status(None, 0, None, None) == errno.EINVAL
    d.lthip_repack_destroy(None)
