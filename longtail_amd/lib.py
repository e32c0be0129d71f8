"""ctypes binding of liblongtail_hip.so (include/longtail_hip.h) + thin torch-tensor conveniences.

Nothing here computes anything on the CPU: every call goes through the C ABI into the HIP kernels, and loading
fails loudly when the library (or a GPU, for the compute entry points) is missing.
"""
from __future__ import annotations

import ctypes as C
import errno
import os
from pathlib import Path
from typing import Optional, Sequence

import numpy as np

# (LTHIP_LIB_PATH: another build of the same sources next to the in-tree one, for same-box A/B runs of compile-time constants)
_LIB_PATH = Path(os.environ["LTHIP_LIB_PATH"]) if os.environ.get("LTHIP_LIB_PATH") else Path(__file__).resolve().parent / "liblongtail_hip.so"

KERNEL_IDS = {
    "buzhash": 0,
    "select": 1,
    "compact": 2,
    "blake3_leaf": 3,
    "blake3_parent": 4,
    "lz4_segments": 5,
    "lz4_stitch": 6,
    "other": 7,
    "zstd_encode": 8,
    "gather": 9,
}
# BLAKE2s ('blk2') kernels, kept out of KERNEL_IDS (bench.py reports every key of that dict): read with Context.timing_get_blake2s()
BLAKE2S_KERNEL_ID = 10
HASH_BLAKE3 = 0x626C6B33  # 'blk3', lib/blake3/longtail_blake3.c
HASH_BLAKE2 = 0x626C6B32  # 'blk2', lib/blake2/longtail_blake2.c
B3_STREAM_BATCH = 1 << 20  # include/longtail_hip.h LTHIP_B3_STREAM_BATCH
B3_STREAM_STACK_BYTES = 2048
B2S_STREAM_BATCH = 1 << 20  # include/longtail_hip.h LTHIP_B2S_STREAM_BATCH
B2S_STREAM_STATE_BYTES = 64
HASH_MEOW = 0x6D656F77  # 'meow', lib/meowhash/longtail_meowhash.c
MEOW_STREAM_BATCH = 1 << 20  # include/longtail_hip.h LTHIP_MEOW_STREAM_BATCH
MEOW_STREAM_STATE_BYTES = 136


class LongtailHipError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str = ""):
        self.code = code
        super().__init__(f"{what}: errno {code} ({errno.errorcode.get(code, '?')}) {detail}")


def _u64arr(a: Sequence[int]) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _u32arr(a: Sequence[int]) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32))


ABI_VERSION = 4  # include/longtail_hip.h LTHIP_ABI_VERSION


class HipLib:
    """The loaded shared library with argtypes/restypes set."""

    def __init__(self, path: Optional[os.PathLike] = None):
        p = Path(path) if path else _LIB_PATH
        if not p.exists():
            raise FileNotFoundError(
                f"{p} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` or `make` first "
                "(there is no CPU fallback)"
            )
        self.path = p
        # torch bundles its own HIP/HSA runtime; when it is going to be used in this process it must be loaded
        # first so that the library binds to the SAME runtime (two runtimes in one process -> no devices).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        self.dll = C.CDLL(str(p))
        d = self.dll
        vp, u64, u32, i32, sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_size_t
        P = C.POINTER

        def sig(name, res, args):
            f = getattr(d, name)
            f.restype = res
            f.argtypes = args
            return f

        # --- plugin constructors ---
        sig("Longtail_CreateHipChunkerAPI", vp, [])
        sig("Longtail_CreateHipBlake3HashAPI", vp, [])
        sig("Longtail_CreateHipBlake2HashAPI", vp, [])
        sig("Longtail_CreateHipMeowHashAPI", vp, [])
        sig("Longtail_CreateHipLZ4CompressionAPI", vp, [])
        sig("Longtail_CompressionRegistry_CreateForHipLZ4", vp, [u32, P(u32)])
        sig("Longtail_GetHipLZ4DefaultQuality", u32, [])
        sig("Longtail_CreateHipZStdCompressionAPI", vp, [])
        sig("Longtail_CompressionRegistry_CreateForHipZstd", vp, [u32, P(u32)])
        sig("Longtail_Hip_SetAllocator", None, [vp, vp])
        sig("Longtail_Hip_SetDevice", i32, [i32])
        sig("Longtail_Hip_GetLastError", i32, [])
        sig("Longtail_Hip_PinnedBytes", u64, [])
        sig("Longtail_Hip_BatchStats", None, [vp, vp])
        sig("Longtail_Hip_MemoStats", None, [vp, vp])
        # --- bulk API ---
        sig("lthip_ctx_create", i32, [i32, vp, P(vp)])
        sig("lthip_ctx_destroy", None, [vp])
        sig("lthip_ctx_sync", i32, [vp])
        sig("lthip_ctx_error", C.c_char_p, [vp])
        sig("lthip_device_count", i32, [])
        sig("lthip_build_id", C.c_char_p, [])
        sig("lthip_abi_version", i32, [])
        if d.lthip_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{p}: binary interface version {d.lthip_abi_version()}, this binding was written for {ABI_VERSION} "
                               "(include/longtail_hip.h LTHIP_ABI_VERSION): rebuild the library")
        sig("lthip_malloc_device", i32, [vp, sz, P(vp)])
        sig("lthip_free_device", None, [vp, vp])
        sig("lthip_malloc_pinned", i32, [vp, sz, P(vp)])
        sig("lthip_free_pinned", None, [vp, vp])
        sig("lthip_copy_h2d", i32, [vp, vp, vp, sz])
        sig("lthip_copy_d2h", i32, [vp, vp, vp, sz])
        sig("lthip_link_copy", i32, [vp, vp, vp, sz])
        sig("lthip_timing_enable", i32, [vp, i32])
        sig("lthip_timing_reset", i32, [vp])
        sig("lthip_timing_get", i32, [vp, i32, P(C.c_double), P(u64)])
        sig("lthip_plan_create", i32, [vp, u32, vp, vp, u32, u32, u32, P(vp)])
        sig("lthip_plan_destroy", None, [vp, vp])
        sig("lthip_plan_resize_single", i32, [vp, vp, u64])
        sig("lthip_plan_chunk_capacity", u64, [vp])
        sig("lthip_plan_slices", u32, [vp])
        sig("lthip_plan_walked_scans", u32, [vp])
        sig("lthip_chunk_hash", i32, [vp, vp, vp, vp, vp, vp, vp, P(u64)])
        sig("lthip_chunk_from_buffer", i32, [vp, vp, u64, u32, u32, u32, P(u64)])
        sig("lthip_hash_ranges", i32, [vp, vp, u64, vp, vp, u32, vp])
        sig("lthip_lz4_bound", sz, [sz])
        sig("lthip_lz4_compress_blocks", i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp, i32])
        sig("lthip_lz4_decompress_blocks", i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp])
        sig("lthip_zstd_bound", sz, [sz])
        sig("lthip_zstd_compress_blocks", i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp])
        sig("lthip_zstd_compress_blocks_q", i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp, i32])
        sig("lthip_zstd_quality_of_settings", i32, [u32])
        sig("lthip_zstd_decompress_blocks", i32, [vp, vp, u32, vp, vp, vp, vp, vp, vp])
        sig("lthip_zstd_debug_units", i32, [vp, u64, u64, vp, vp, vp])
        sig("lthip_zstd_last_decode_stats", i32, [vp, vp])
        sig("lthip_debug_reload_env", None, [])
        sig("lthip_debug_fail_alloc", i32, [C.c_int64, C.c_int64])
        sig("lthip_debug_alloc_calls", C.c_int64, [P(C.c_int64)])
        sig("lthip_debug_walk_tiles", i32, [P(C.c_uint64)])
        sig("lthip_stored_block_header_size", sz, [u32])
        sig("lthip_write_stored_block_headers", i32, [vp, u32, vp, vp, vp, u32, u32, vp, vp, vp, vp])
        sig("lthip_block_index_size", sz, [u32])
        sig("lthip_write_raw_block_images", i32, [vp, u32, vp, vp, vp, vp, vp, u32, vp, vp])
        sig("lthip_create_missing_content", i32, [vp, u64, vp, u64, vp, vp, vp, u32, u32, u32, vp, sz, vp])
        sig("lthip_get_existing_store_index", i32, [vp, vp, sz, u64, vp, u32, vp, sz, vp])
        sig("lthip_version_index_size", sz, [u32, u64, u64, u32])
        sig("lthip_build_version_index", i32, [vp, u32, vp, vp, vp, vp, u32, vp, u64, vp, vp, vp, u32, u32, vp, sz, vp])
        sig("lthip_dedup_first_seen", i32, [vp, u64, vp, vp, vp])
        sig("lthip_dedup_min_ordinal", i32, [vp, u64, vp, vp, vp, vp])
        sig("lthip_seen_create", i32, [vp, u64, P(vp)])
        sig("lthip_seen_destroy", None, [vp])
        sig("lthip_seen_add", i32, [vp, u64, vp, vp, vp])
        sig("lthip_seen_total", u64, [vp])
        sig("lthip_seen_grown", u64, [vp])
        sig("lthip_seen_find", i32, [vp, u64, vp, vp])
        sig("lthip_restore_layout", i32, [vp, sz, u64, vp, P(u32), P(u64)])
        sig("lthip_restore_create", i32, [vp, vp, vp, sz, vp, sz, vp, u64, P(vp)])
        sig("lthip_restore_destroy", None, [vp])
        sig("lthip_restore_needed_blocks", i32, [vp, vp, u64, P(u64)])
        sig("lthip_restore_scratch_bound", sz, [vp, u32, vp])
        sig("lthip_restore_blocks", i32, [vp, u32, vp, vp, vp, vp, vp, u64, vp])
        sig("lthip_restore_finish", i32, [vp, vp])
        sig("lthip_restore_block_status", i32, [vp, u32, vp, vp])
        sig("lthip_restore_create_from_base", i32, [vp, vp, vp, vp, sz, vp, sz, vp, u64, P(vp)])
        sig("lthip_restore_carry", i32, [vp, vp, vp])
        sig("lthip_version_diff", i32, [vp, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp])
        sig("lthip_restore_layout_in_place", i32, [vp, sz, vp, u64, vp, sz, u64, vp, P(u32), P(u64), P(u32)])
        sig("lthip_restore_in_place_scratch_bound", sz, [vp])
        sig("lthip_restore_in_place_stats", i32, [vp, vp])
        sig("lthip_restore_carry_in_place", i32, [vp, vp, vp, u64])
        sig("lthip_restore_create_windows", i32, [vp, vp, vp, sz, vp, sz, u64, vp, u64, P(vp)])
        sig("lthip_restore_asset_sizes", i32, [vp, sz, vp, P(u32), P(u32)])
        sig("lthip_restore_rank_windows", i32, [u64, vp, vp, vp, vp, u32, u64, vp, u64, P(u64), P(u64)])
        sig("lthip_block_cache_create", i32, [vp, u32, u64, P(vp)])
        sig("lthip_block_cache_destroy", None, [vp])
        sig("lthip_block_cache_contains", i32, [vp, u32, u32, vp, vp])
        sig("lthip_block_cache_clear", i32, [vp])
        sig("lthip_block_cache_stats", i32, [vp, vp])
        sig("lthip_restore_set_cache", i32, [vp, vp])
        sig("lthip_restore_from_cache", i32, [vp, vp])
        sig("lthip_restore_cache_stats", i32, [vp, vp])
        sig("lthip_archive_index_size", i32, [vp, sz, vp, sz, P(u64)])
        sig("lthip_archive_write_index", i32, [vp, sz, vp, sz, vp, vp, vp, sz])
        sig("lthip_archive_peek", i32, [vp, P(u64)])
        sig("lthip_archive_open", i32, [vp, sz, u64, P(vp)])
        sig("lthip_archive_close", None, [vp])
        sig("lthip_archive_store_index", vp, [vp, P(sz)])
        sig("lthip_archive_version_index", vp, [vp, P(sz)])
        sig("lthip_archive_block_count", u32, [vp])
        sig("lthip_archive_block_offsets", vp, [vp])
        sig("lthip_archive_block_sizes", vp, [vp])
        sig("lthip_archive_body_bytes", u64, [vp])
        sig("lthip_archive_writer_create", i32, [vp, P(vp)])
        sig("lthip_archive_writer_destroy", None, [vp])
        sig("lthip_archive_writer_append", i32, [vp, vp, u32, vp, vp, vp, u64, P(u64)])
        sig("lthip_archive_writer_blocks", i32, [vp, P(u64), P(vp), P(vp), P(u64)])
        sig("lthip_archive_writer_finish", i32, [vp, vp, sz, vp, sz, vp, sz, P(u64)])
        sig("lthip_restore_archive_blocks", i32, [vp, vp, vp, u64, u64, vp, u64, vp, P(u32), P(u64)])
        sig("lthip_restore_archive_scratch_bound", sz, [vp, vp, u64, u64])
        sig("lthip_restore_archive_ranges", i32, [vp, vp, u64, vp, u64, P(u64)])
        sig("lthip_store_index_prune", i32, [vp, sz, u32, vp, vp, sz, P(sz)])
        sig("lthip_store_index_merge", i32, [vp, sz, vp, sz, vp, sz, P(sz)])
        sig("lthip_version_chunk_hashes", i32, [vp, sz, vp, u64, P(u64)])
        sig("lthip_repack_create", i32, [vp, vp, vp, sz, u64, vp, P(vp)])
        sig("lthip_repack_destroy", None, [vp])
        sig("lthip_repack_plan_info", i32, [vp, vp])
        for name in ("kept", "dropped", "source"):
            sig(f"lthip_repack_{name}_blocks", i32, [vp, vp, u64, P(u64)])
        sig("lthip_repack_kept_index", i32, [vp, vp, sz, P(sz)])
        sig("lthip_repack_scratch_bound", sz, [vp, u32, vp])
        sig("lthip_repack_blocks", i32, [vp, u32, vp, vp, vp, vp, vp, u64, vp])
        sig("lthip_repack_write", i32, [vp, vp, u64])
        sig("lthip_repack_finish", i32, [vp, vp, sz, P(sz), vp])
        sig("lthip_repack_images", i32, [vp, P(u64), P(vp), P(vp)])
        sig("lthip_repack_store_index", i32, [vp, vp, sz, P(sz)])
        sig("lthip_repack_block_status", i32, [vp, u32, vp, vp])
        sig("lthip_store_create", i32, [vp, u64, P(vp)])
        sig("lthip_store_destroy", None, [vp])
        sig("lthip_store_add", i32, [vp, u64, vp])
        sig("lthip_store_add_index", i32, [vp, vp, sz])
        sig("lthip_store_find", i32, [vp, u64, vp, vp, vp])
        sig("lthip_store_added", u64, [vp])
        sig("lthip_store_distinct", i32, [vp, P(u64)])
        sig("lthip_store_grown", u64, [vp])
        sig("lthip_ingest_set_first_seen", i32, [vp, vp, u64])
        sig("lthip_ingest_set_store", i32, [vp, vp])
        sig("lthip_ingest_store_stats", i32, [vp, P(u64), P(u64)])
        sig("lthip_plan_reaim", i32, [vp, vp, u32, vp, vp])
        sig("lthip_hash_one", i32, [vp, vp, u32, vp])
        sig("lthip_hash_runs_u64", i32, [vp, vp, vp, u32, vp])
        sig("lthip_hash_runs_u64_bounded", i32, [vp, vp, vp, u32, u64, u64, vp])
        sig("lthip_b3_stream_batch", i32, [vp, vp, u64, vp])
        sig("lthip_b3_stream_final", i32, [vp, vp, u32, u64, vp, vp])
        for name, stream in (("lthip_blake2s", "lthip_b2s_stream"), ("lthip_meow", "lthip_meow_stream")):  # the chain hashes
            sig(name + "_ranges", i32, [vp, vp, u64, vp, vp, u32, vp])
            sig(name + "_ranges_dev", i32, [vp, vp, u64, vp, vp, vp, u32, vp])
            sig(name + "_one", i32, [vp, vp, u32, vp])
            sig(name + "_runs_u64", i32, [vp, vp, vp, u32, vp])
            sig(name + "_runs_u64_bounded", i32, [vp, vp, vp, u32, u64, u64, vp])
            sig(stream + "_batch", i32, [vp, vp, u64, vp])
            sig(stream + "_final", i32, [vp, vp, u32, u64, vp, vp])
        sig("lthip_dedup_first_seen_range", i32, [vp, u64, vp, u64, u64, vp, vp])
        sig("lthip_gather_ranges", i32, [vp, vp, u64, vp, vp, vp, vp])
        sig("lthip_pack_blocks", i32, [u64, vp, u32, u32, vp, u64, P(u64)])
        sig("lthip_pack_blocks_batch", i32, [u64, vp, u64, u32, u32, u64, u64, u32, u32, vp, vp, u64, P(u64), P(u64)])
        sig("lthip_synth_fill", i32, [vp, vp, u32, vp, vp, vp, i32])
        sig("lthip_synth_fill_ranges", i32, [vp, vp, u32, vp, vp, vp, vp, i32])
        sig("lthip_ingest_create", i32, [vp, vp, P(vp)])
        sig("lthip_ingest_destroy", None, [vp])
        sig("lthip_ingest_index", i32, [vp, vp, vp, vp, u64, vp, vp, u64, vp, sz])
        sig("lthip_ingest_write", i32, [vp, vp, vp, u64])
        sig("lthip_ingest_finish", i32, [vp, vp, sz, vp])
        sig("lthip_ingest_compressed_sizes", vp, [vp])
        sig("lthip_ingest_images", i32, [vp, P(u64), P(u64), P(vp), P(vp)])
        sig("lthip_ingest_stream_create", i32, [vp, vp, vp, P(vp)])
        sig("lthip_ingest_stream_destroy", None, [vp])
        sig("lthip_ingest_stream_arena_bound", sz, [vp, u64, u64])
        sig("lthip_ingest_stream_slice", i32, [vp, u64, u64, vp, vp, vp, vp, vp, u64, vp, u64])
        sig("lthip_ingest_stream_images", i32, [vp, P(u64), P(u64), P(vp), P(vp)])
        sig("lthip_ingest_stream_finish", i32, [vp, vp, u64, vp, sz, vp, sz, vp])
        sig("lthip_ingest_stream_table_grown", u64, [vp])
        sig("lthip_ingest_stream_set_store", i32, [vp, vp])
        sig("lthip_ingest_stream_store_stats", i32, [vp, P(u64), P(u64)])
        sig("lthip_divtest_eval", i32, [u32, u32])
        sig("lthip_job_count", u64, [u32, vp, u32])
        sig("lthip_make_jobs", i32, [u32, vp, u32, u64, vp, vp, vp])
        sig("lthip_partition_jobs", i32, [u64, vp, u32, i32, vp, vp])
        sig("lthip_exchange_layout", i32, [u64, vp, u32, vp, u64, u64, vp, vp, vp])
        sig("lthip_exchange_ranges", u64, [u64, vp, vp, vp, u64, u64, vp, vp, vp])
        sig("lthip_exchange_reorder", i32, [vp, vp, vp, u32, u64, vp, vp, vp])
        sig("lthip_job_ordinals", i32, [vp, u64, vp, vp, u64, vp])
        sig("lthip_comm_unique_id", i32, [vp])
        sig("lthip_comm_create", i32, [vp, i32, i32, vp, P(vp)])
        sig("lthip_comm_destroy", i32, [vp])
        sig("lthip_comm_allgather", i32, [vp, vp, vp, vp, u64, u32])
        sig("lthip_comm_alltoallv", i32, [vp, vp, vp, vp, vp, vp, vp, vp, u32])
        sig("lthip_comm_info", i32, [vp, P(i32), P(i32), P(i32)])

    def device_count(self) -> int:
        return int(self.dll.lthip_device_count())

    def build_id(self) -> str:
        return self.dll.lthip_build_id().decode()


_lib: Optional[HipLib] = None


ABLATIONS_LIB_PATH = Path(__file__).resolve().parent.parent / "build" / "ablations" / "liblongtail_hip.so"
_abl = None


def load_ablations() -> HipLib:
    """The ABLATION build of the same sources (`make ablations`: -DLTHIP_ABLATIONS): earlier formulations of the kernels and debug
    paths behind LTHIP_* switches, kept as second implementations for the differential tests and the A/B tools.  The product
    library has none of them.  A separate handle: load() keeps returning the product library."""
    global _abl
    if _abl is None:
        if os.environ.get("LTHIP_LIB_PATH"):
            _abl = load()  # (the whole process runs on the library named there)
        else:
            if not ABLATIONS_LIB_PATH.exists():
                raise FileNotFoundError(f"{ABLATIONS_LIB_PATH} is missing: run `make ablations` (or __graft_entry__.build())")
            _abl = HipLib(ABLATIONS_LIB_PATH)
    return _abl


def load(path: Optional[os.PathLike] = None) -> HipLib:
    global _lib
    if _lib is None or path is not None:
        _lib = HipLib(path)
    return _lib


def _ptr(t) -> int:
    """device/host pointer of a torch tensor or numpy array (0 for None)."""
    if t is None:
        return 0
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return int(t.data_ptr())


class Context:
    """One lthip_ctx bound to a torch device and (by default) torch's current stream on it."""

    def __init__(self, device: int = 0, stream: "object | None" = "torch", lib: Optional[HipLib] = None):
        import torch

        self.lib = lib or load()
        self.torch = torch
        self.device = device
        if stream == "torch":
            raw_stream = int(torch.cuda.current_stream(device).cuda_stream)  # 0 = the null stream, also valid
        elif stream is None:
            raw_stream = -1  # LTHIP_STREAM_PRIVATE
        else:
            raw_stream = int(stream)
        h = C.c_void_p()
        err = self.lib.dll.lthip_ctx_create(device, C.c_void_p(raw_stream), C.byref(h))
        if err:
            raise LongtailHipError(err, "lthip_ctx_create", "(no GPU?)" if err == errno.ENODEV else "")
        self.h = h

    # -- plumbing --
    def close(self):
        if getattr(self, "h", None):
            self.lib.dll.lthip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, err: int, what: str):
        if err:
            msg = self.lib.dll.lthip_ctx_error(self.h)
            raise LongtailHipError(err, what, msg.decode() if msg else "")

    def sync(self):
        self._check(self.lib.dll.lthip_ctx_sync(self.h), "lthip_ctx_sync")

    def timing(self, on: bool):
        self._check(self.lib.dll.lthip_timing_enable(self.h, 1 if on else 0), "lthip_timing_enable")

    def timing_reset(self):
        self._check(self.lib.dll.lthip_timing_reset(self.h), "lthip_timing_reset")

    def timing_get(self) -> dict:
        out = {}
        for name, kid in KERNEL_IDS.items():
            ms, n = C.c_double(0), C.c_uint64(0)
            self._check(self.lib.dll.lthip_timing_get(self.h, kid, C.byref(ms), C.byref(n)), "lthip_timing_get")
            out[name] = (ms.value, n.value)
        return out

    def _dev(self):
        return self.torch.device("cuda", self.device)

    # -- synthetic data --
    def synth_fill(self, dst, offsets, sizes, seeds, kind: int, skips=None):
        """Ranges [skips[i], skips[i] + sizes[i]) of the assets with the given seeds -> dst + offsets[i] (include/longtail_synth.h)."""
        o, s, sd = _u64arr(offsets), _u64arr(sizes), _u64arr(seeds)
        sk = _u64arr(skips) if skips is not None else None
        self._check(
            self.lib.dll.lthip_synth_fill_ranges(self.h, _ptr(dst), len(o), o.ctypes.data, s.ctypes.data, sd.ctypes.data,
                                                 sk.ctypes.data if sk is not None else None, kind),
            "lthip_synth_fill_ranges",
        )

    # -- phase 1 --
    def make_plan(self, part_offsets, part_sizes, min_chunk: int, avg_chunk: int, max_chunk: int) -> "Plan":
        return Plan(self, part_offsets, part_sizes, min_chunk, avg_chunk, max_chunk)

    def chunk_hash(self, plan: "Plan", data, want_hashes: bool = True, outputs=None, sync: bool = True):
        """-> (total, offsets u64[cap], lens u32[cap], hashes u64[cap] | None, part_first u32[nparts+1]) torch tensors."""
        torch = self.torch
        cap = max(1, plan.capacity)
        if outputs is None:
            dev = self._dev()
            offs = torch.empty(cap, dtype=torch.int64, device=dev)
            lens = torch.empty(cap, dtype=torch.int32, device=dev)
            hashes = torch.empty(cap, dtype=torch.int64, device=dev) if want_hashes else None
            first = torch.empty(plan.nparts + 1, dtype=torch.int32, device=dev)
        else:
            offs, lens, hashes, first = outputs
        total = C.c_uint64(0)
        err = self.lib.dll.lthip_chunk_hash(
            self.h, plan.h, _ptr(data), _ptr(offs), _ptr(lens), _ptr(hashes), _ptr(first), C.byref(total) if sync else None
        )
        self._check(err, "lthip_chunk_hash")
        return (int(total.value) if sync else None), offs, lens, hashes, first

    def hash_ranges(self, data, offsets, lens, max_len: int = 0, out=None):
        torch = self.torch
        n = int(offsets.numel())
        if out is None:
            out = torch.empty(max(1, n), dtype=torch.int64, device=self._dev())
        self._check(
            self.lib.dll.lthip_hash_ranges(self.h, _ptr(data), n, _ptr(offsets), _ptr(lens), max_len, _ptr(out)),
            "lthip_hash_ranges",
        )
        return out[:n]

    def hash_one(self, data, length: int, out) -> None:
        """BLAKE3-64 of one input of at most 64 KiB (device or pinned memory, any alignment); the digest lands in `out` (device or
        pinned) on the stream."""
        self._check(self.lib.dll.lthip_hash_one(self.h, _ptr(data), length, _ptr(out)), "lthip_hash_one")

    def hash_runs_u64(self, values, first, run_count: int, out=None):
        """out[i] = BLAKE3-64 of the bytes of values[first[i] .. first[i + 1]) (device u64 / u32 tensors)."""
        if out is None:
            out = self.torch.empty(max(1, run_count), dtype=self.torch.int64, device=self._dev())
        self._check(self.lib.dll.lthip_hash_runs_u64(self.h, _ptr(values), _ptr(first), run_count, _ptr(out)), "lthip_hash_runs_u64")
        return out[:run_count]

    def hash_runs_u64_bounded(self, values, first, run_count: int, total_values_bound: int, run_values_bound: int, out=None):
        """hash_runs_u64 with the caller's upper bounds of all values and of the longest run (0 = unknown): no read-back."""
        if out is None:
            out = self.torch.empty(max(1, run_count), dtype=self.torch.int64, device=self._dev())
        self._check(self.lib.dll.lthip_hash_runs_u64_bounded(self.h, _ptr(values), _ptr(first), run_count, total_values_bound, run_values_bound,
                                                             _ptr(out)), "lthip_hash_runs_u64_bounded")
        return out[:run_count]

    def b3_stream(self, data, length: int) -> int:
        """Streaming BLAKE3-64 of the first `length` bytes of a device tensor, batch by batch (lthip_b3_stream_batch / _final)."""
        return self._chain_stream("lthip_b3_stream", B3_STREAM_BATCH, B3_STREAM_STACK_BYTES, data, length)

    # -- the chain hashes: BLAKE2s-64 ('blk2') and Meow hash v0.5, 64 bits ('meow'); `name` is the prefix of the kind's C calls --
    def _chain_ranges(self, name, data, offsets, lens, max_len, out, count_bound, d_count):
        torch = self.torch
        n = int(offsets.numel()) if count_bound is None else int(count_bound)
        if out is None:
            out = torch.empty(max(1, n), dtype=torch.int64, device=self._dev())
        if d_count is None:
            err = getattr(self.lib.dll, name + "_ranges")(self.h, _ptr(data), n, _ptr(offsets), _ptr(lens), max_len, _ptr(out))
        else:
            err = getattr(self.lib.dll, name + "_ranges_dev")(self.h, _ptr(data), n, _ptr(d_count), _ptr(offsets), _ptr(lens), max_len, _ptr(out))
        self._check(err, name + "_ranges")
        return out[:n]

    def _chain_one(self, name, data, length, out) -> None:
        self._check(getattr(self.lib.dll, name + "_one")(self.h, _ptr(data), length, _ptr(out)), name + "_one")

    def _chain_runs_u64(self, name, values, first, run_count, out):
        if out is None:
            out = self.torch.empty(max(1, run_count), dtype=self.torch.int64, device=self._dev())
        self._check(getattr(self.lib.dll, name + "_runs_u64")(self.h, _ptr(values), _ptr(first), run_count, _ptr(out)), name + "_runs_u64")
        return out[:run_count]

    def _chain_stream(self, name, batch_bytes, state_bytes, data, length) -> int:
        torch = self.torch
        state = torch.empty(state_bytes, dtype=torch.uint8, device=self._dev())
        out = torch.zeros(1, dtype=torch.int64, device=self._dev())
        base = _ptr(data)
        batches = max(0, (length - 1) // batch_bytes)
        for b in range(batches):
            self._check(getattr(self.lib.dll, name + "_batch")(self.h, base + b * batch_bytes, b, _ptr(state)), name + "_batch")
        tail = length - batches * batch_bytes
        self._check(getattr(self.lib.dll, name + "_final")(self.h, base + batches * batch_bytes if tail else None, tail, batches, _ptr(state),
                                                           _ptr(out)), name + "_final")
        return int(out.cpu().numpy().view(np.uint64)[0])

    def blake2s_ranges(self, data, offsets, lens, max_len: int = 0, out=None, count_bound: Optional[int] = None, d_count=None):
        """d_hashes[i] = blake2s-64 of the range; with d_count (device u32) the number of ranges is min(count_bound, *d_count)."""
        return self._chain_ranges("lthip_blake2s", data, offsets, lens, max_len, out, count_bound, d_count)

    def blake2s_one(self, data, length: int, out) -> None:
        """One input of at most 64 KiB (device or pinned memory); the digest lands in `out` (device or pinned) on the stream."""
        self._chain_one("lthip_blake2s", data, length, out)

    def blake2s_runs_u64(self, values, first, run_count: int, out=None):
        return self._chain_runs_u64("lthip_blake2s", values, first, run_count, out)

    def b2s_stream(self, data, length: int) -> int:
        """Streaming BLAKE2s-64 of the first `length` bytes of a device tensor, batch by batch (lthip_b2s_stream_batch / _final)."""
        return self._chain_stream("lthip_b2s_stream", B2S_STREAM_BATCH, B2S_STREAM_STATE_BYTES, data, length)

    def meow_ranges(self, data, offsets, lens, max_len: int = 0, out=None, count_bound: Optional[int] = None, d_count=None):
        """d_hashes[i] = meow-64 of the range; with d_count (device u32) the number of ranges is min(count_bound, *d_count)."""
        return self._chain_ranges("lthip_meow", data, offsets, lens, max_len, out, count_bound, d_count)

    def meow_one(self, data, length: int, out) -> None:
        """One input of at most 64 KiB (device or pinned memory); the digest lands in `out` (device or pinned) on the stream."""
        self._chain_one("lthip_meow", data, length, out)

    def meow_runs_u64(self, values, first, run_count: int, out=None):
        return self._chain_runs_u64("lthip_meow", values, first, run_count, out)

    def meow_stream(self, data, length: int) -> int:
        """Streaming meow-64 of the first `length` bytes of a device tensor, batch by batch (lthip_meow_stream_batch / _final)."""
        return self._chain_stream("lthip_meow_stream", MEOW_STREAM_BATCH, MEOW_STREAM_STATE_BYTES, data, length)

    def timing_get_blake2s(self):
        """(total ms, launches) of the BLAKE2s kernels since the last timing_reset."""
        ms, n = C.c_double(0), C.c_uint64(0)
        self._check(self.lib.dll.lthip_timing_get(self.h, BLAKE2S_KERNEL_ID, C.byref(ms), C.byref(n)), "lthip_timing_get")
        return ms.value, n.value

    def chunk_from_buffer(self, data, size: int, min_chunk: int, avg_chunk: int, max_chunk: int) -> int:
        out = C.c_uint64(0)
        self._check(
            self.lib.dll.lthip_chunk_from_buffer(self.h, _ptr(data), size, min_chunk, avg_chunk, max_chunk, C.byref(out)),
            "lthip_chunk_from_buffer",
        )
        return int(out.value)

    # -- phase 2 --
    def _codec(self, fn, src, src_offsets, src_sizes, dst, dst_offsets, dst_caps, extra=()):
        torch = self.torch
        so, ss = _u64arr(src_offsets), _u32arr(src_sizes)
        do, dc = _u64arr(dst_offsets), _u32arr(dst_caps)
        n = len(so)
        out_sizes = torch.empty(max(1, n), dtype=torch.int32, device=self._dev())
        err = fn(self.h, _ptr(src), n, so.ctypes.data, ss.ctypes.data, _ptr(dst), do.ctypes.data, dc.ctypes.data,
                 _ptr(out_sizes), *extra)
        self._check(err, fn.__name__)
        return out_sizes[:n]

    def lz4_compress_blocks(self, src, src_offsets, src_sizes, dst, dst_offsets, dst_caps, segment_log2: int = 0):
        return self._codec(self.lib.dll.lthip_lz4_compress_blocks, src, src_offsets, src_sizes, dst, dst_offsets,
                           dst_caps, (segment_log2,))

    def lz4_decompress_blocks(self, src, src_offsets, src_sizes, dst, dst_offsets, dst_caps):
        return self._codec(self.lib.dll.lthip_lz4_decompress_blocks, src, src_offsets, src_sizes, dst, dst_offsets,
                           dst_caps)

    def zstd_compress_blocks(self, src, src_offsets, src_sizes, dst, dst_offsets, dst_caps, quality: int = 0):
        """quality: 0 default ('ztd1', 'ztd2'), 1 high ('ztd4'), 2 max ('ztd3', 'ztd5') -- LTHIP_ZSTD_Q_*"""
        return self._codec(self.lib.dll.lthip_zstd_compress_blocks_q, src, src_offsets, src_sizes, dst, dst_offsets,
                           dst_caps, (int(quality),))

    def zstd_decompress_blocks(self, src, src_offsets, src_sizes, dst, dst_offsets, dst_caps):
        return self._codec(self.lib.dll.lthip_zstd_decompress_blocks, src, src_offsets, src_sizes, dst, dst_offsets,
                           dst_caps)

    def zstd_last_decode_stats(self):
        """(payloads, blocks of other encoders' frames listed for the block-parallel decoder, payloads given back to the serial
        decoder) of the last zstd_decompress_blocks call."""
        out = np.zeros(4, np.uint32)
        self._check(self.lib.dll.lthip_zstd_last_decode_stats(self.h, out.ctypes.data), "lthip_zstd_last_decode_stats")
        return tuple(int(v) for v in out)

    def zstd_debug_units(self, first: int, count: int):
        """Match-finder output of the last zstd_compress_blocks call: (meta[count,4] u32, lits[count,4096] u8,
        recs[count,1024] u64) for the 4 KiB units [first, first+count)."""
        meta = np.zeros((count, 4), np.uint32)
        lits = np.zeros((count, 4096), np.uint8)
        recs = np.zeros((count, 1024), np.uint64)
        self._check(self.lib.dll.lthip_zstd_debug_units(self.h, first, count, meta.ctypes.data, lits.ctypes.data,
                                                        recs.ctypes.data), "lthip_zstd_debug_units")
        return meta, lits, recs

    def build_version_index(self, asset_sizes, path_start_offsets, permissions, path_data: bytes, asset_chunk_counts,
                            chunk_hashes, chunk_lens, chunk_total: int, target_chunk_size: int, asset_tags=None,
                            hash_identifier: int = 0x626C6B33) -> bytes:
        """Serialized VersionIndex (== Longtail_WriteVersionIndexToBuffer) from device chunk lists; see longtail_hip.h."""
        n = len(asset_sizes)
        a_sz, a_off = _u64arr(asset_sizes), _u32arr(path_start_offsets)
        a_perm = np.ascontiguousarray(np.asarray(permissions, dtype=np.uint16))
        a_cnt = _u32arr(asset_chunk_counts)
        a_tag = _u32arr(asset_tags) if asset_tags is not None else None
        cap = self.lib.dll.lthip_version_index_size(n, chunk_total, chunk_total, len(path_data))
        out = np.zeros(cap + 16, np.uint8)
        size = C.c_size_t(0)
        err = self.lib.dll.lthip_build_version_index(
            self.h, n, a_sz.ctypes.data, a_off.ctypes.data, a_perm.ctypes.data, path_data, len(path_data), a_cnt.ctypes.data,
            chunk_total, _ptr(chunk_hashes), _ptr(chunk_lens), a_tag.ctypes.data if a_tag is not None else None, hash_identifier,
            target_chunk_size, out.ctypes.data, cap, C.byref(size))
        self._check(err, "lthip_build_version_index")
        return out[: size.value].tobytes()

    def write_stored_block_headers(self, block_first_chunk, chunk_hashes, chunk_lens, tag: int, raw_sizes, comp_sizes, arena,
                                   image_offsets, hash_identifier: int = 0x626C6B33):
        """BlockIndex + [raw][compressed] size words around payloads already compressed into `arena` (see longtail_hip.h)."""
        bf, rs, io = _u64arr(block_first_chunk), _u32arr(raw_sizes), _u64arr(image_offsets)
        self._check(self.lib.dll.lthip_write_stored_block_headers(self.h, len(io), bf.ctypes.data, _ptr(chunk_hashes), _ptr(chunk_lens),
                                                                  hash_identifier, tag, rs.ctypes.data, _ptr(comp_sizes), _ptr(arena),
                                                                  io.ctypes.data), "lthip_write_stored_block_headers")

    def block_index_size(self, chunk_count: int) -> int:
        """bytes of a BlockIndex of that many chunks: what lies in front of the chunks' bytes in a raw (tag 0) block image"""
        return int(self.lib.dll.lthip_block_index_size(chunk_count))

    def write_raw_block_images(self, block_first_chunk, chunk_hashes, chunk_lens, chunk_src_offsets, src, arena, image_offsets,
                               hash_identifier: int = 0x626C6B33):
        """The complete tag-0 images -- BlockIndex + the chunks' bytes copied from src + chunk_src_offsets[c] -- at `image_offsets` of
        `arena`; asynchronous on the context's stream (see longtail_hip.h)."""
        bf, io = _u64arr(block_first_chunk), _u64arr(image_offsets)
        self._check(self.lib.dll.lthip_write_raw_block_images(self.h, len(io), bf.ctypes.data, _ptr(chunk_hashes), _ptr(chunk_lens),
                                                              _ptr(chunk_src_offsets), _ptr(src), hash_identifier, _ptr(arena),
                                                              io.ctypes.data), "lthip_write_raw_block_images")

    def create_missing_content(self, existing_hashes, chunk_hashes, chunk_lens, chunk_tags, max_block_size: int,
                               max_chunks_per_block: int, hash_identifier: int = 0x626C6B33) -> bytes:
        """Serialized StoreIndex of the version chunks a store with `existing_hashes` lacks (see longtail_hip.h)."""
        ne = int(existing_hashes.numel()) if existing_hashes is not None else 0
        n = int(chunk_hashes.numel())
        tags = _u32arr(chunk_tags) if chunk_tags is not None else None
        cap = 16 + 20 * n + 12 * n + 64
        out = np.zeros(cap, np.uint8)
        size = C.c_size_t(0)
        err = self.lib.dll.lthip_create_missing_content(
            self.h, ne, _ptr(existing_hashes) if ne else None, n, _ptr(chunk_hashes), _ptr(chunk_lens),
            tags.ctypes.data if tags is not None else None, hash_identifier, max_block_size, max_chunks_per_block, out.ctypes.data,
            cap, C.byref(size))
        self._check(err, "lthip_create_missing_content")
        return out[: size.value].tobytes()

    def get_existing_store_index(self, store_index: bytes, chunk_hashes, min_block_usage_percent: int) -> bytes:
        """Serialized StoreIndex of the store's blocks that cover `chunk_hashes` (device int64/uint64 tensor); see longtail_hip.h."""
        raw = np.frombuffer(store_index, np.uint8)
        n = int(chunk_hashes.numel()) if chunk_hashes is not None else 0
        out = np.zeros(len(raw) + 64, np.uint8)
        size = C.c_size_t(0)
        err = self.lib.dll.lthip_get_existing_store_index(self.h, raw.ctypes.data, len(raw), n, _ptr(chunk_hashes) if n else None,
                                                          min_block_usage_percent, out.ctypes.data, len(out), C.byref(size))
        self._check(err, "lthip_get_existing_store_index")
        return out[: size.value].tobytes()

    # -- block assembly --
    def link_copy(self, dst, src, nbytes: int):
        """dst[:nbytes] = src[:nbytes] by the compute units (pinned host <-> device, either direction; include/longtail_hip.h)."""
        self._check(self.lib.dll.lthip_link_copy(self.h, _ptr(dst), _ptr(src), nbytes), "lthip_link_copy")

    def gather_ranges(self, src, src_offsets, lens, dst, dst_offsets):
        n = int(src_offsets.numel())
        self._check(self.lib.dll.lthip_gather_ranges(self.h, _ptr(src), n, _ptr(src_offsets), _ptr(lens), _ptr(dst),
                                                     _ptr(dst_offsets)), "lthip_gather_ranges")

    def exchange_reorder(self, gathered, out, ranges):
        """out[dst ..) = gathered[src .. + cnt) for the (src, dst, cnt) element ranges of JobPartition.ranges (host arrays)."""
        r_src, r_dst, r_cnt = ranges
        assert gathered.dtype == out.dtype and gathered.is_contiguous() and out.is_contiguous()
        self._check(self.lib.dll.lthip_exchange_reorder(self.h, _ptr(gathered), _ptr(out), gathered.element_size(), len(r_src),
                                                        r_src.ctypes.data, r_dst.ctypes.data, r_cnt.ctypes.data), "lthip_exchange_reorder")

    def job_ordinals(self, local_first: np.ndarray, global_first: np.ndarray, local_chunks: int):
        """int32 tensor [local_chunks]: position in job order of every chunk of this rank (own job m: local_first[m] -> global_first[m])."""
        lf, gf = _u32arr(local_first), _u32arr(global_first)
        assert len(lf) == len(gf)
        out = self.torch.empty(max(1, local_chunks), dtype=self.torch.int32, device=self._dev())
        self._check(self.lib.dll.lthip_job_ordinals(self.h, len(lf), lf.ctypes.data, gf.ctypes.data, local_chunks, _ptr(out)),
                    "lthip_job_ordinals")
        return out[:local_chunks]

    # -- dedup --
    def dedup_first_seen_range(self, hashes, first: int, count: int):
        """All hashes inserted, first-occurrence (global) indices returned for [first, first+count) only; + distinct count."""
        torch = self.torch
        n = int(hashes.numel())
        out = torch.empty(max(1, count), dtype=torch.int32, device=self._dev())
        uniq = torch.zeros(1, dtype=torch.int64, device=self._dev())
        self._check(self.lib.dll.lthip_dedup_first_seen_range(self.h, n, _ptr(hashes), first, count, _ptr(out), _ptr(uniq)),
                    "lthip_dedup_first_seen_range")
        return out[:count], uniq

    def dedup_first_seen(self, hashes):
        torch = self.torch
        n = int(hashes.numel())
        first = torch.empty(max(1, n), dtype=torch.int32, device=self._dev())
        uniq = torch.zeros(1, dtype=torch.int64, device=self._dev())
        self._check(self.lib.dll.lthip_dedup_first_seen(self.h, n, _ptr(hashes), _ptr(first), _ptr(uniq)),
                    "lthip_dedup_first_seen")
        return first[:n], uniq

    def dedup_min_ordinal(self, hashes, ordinals, sync: bool = True):
        """The owner's side of the sharded first-seen table: first[j] = smallest ordinal among the items with the hash of item j
        (int32 tensor), number of distinct hashes (int, after a synchronisation; sync=False: a one-element int64 device tensor)."""
        torch = self.torch
        n = int(hashes.numel())
        first = torch.empty(max(1, n), dtype=torch.int32, device=self._dev())
        uniq = torch.zeros(1, dtype=torch.int64, device=self._dev())
        self._check(self.lib.dll.lthip_dedup_min_ordinal(self.h, n, _ptr(hashes.contiguous()), _ptr(ordinals.contiguous()), _ptr(first), _ptr(uniq)),
                    "lthip_dedup_min_ordinal")
        if not sync:
            return first[:n], uniq
        self.sync()
        return first[:n], int(uniq.item())


class Comm:
    """Communicator behind the C ABI (comm.hip), one process per GPU: RCCL, or -- when the id was made under
    LTHIP_COMM_TRANSPORT=shm -- the shared-memory stand-in for boxes without N GPUs.  `unique_id()` on rank 0, carried to the other
    ranks by the embedder (bench.py: a file, or the torch.distributed store), then `Comm(ctx, nranks, rank, id)` everywhere.
    `ctx=None` (shared-memory transport only): the tensors are CPU tensors (the tests without a GPU)."""

    ID_BYTES = 128
    TRANSPORTS = {1: "rccl", 2: "host-shm"}

    @staticmethod
    def unique_id(lib: Optional[HipLib] = None) -> bytes:
        lib = lib or load()
        buf = (C.c_ubyte * Comm.ID_BYTES)()
        err = lib.dll.lthip_comm_unique_id(C.addressof(buf))
        if err:
            raise LongtailHipError(err, "lthip_comm_unique_id")
        return bytes(buf)

    def __init__(self, ctx: "Optional[Context]", nranks: int, rank: int, unique_id: bytes, lib: Optional[HipLib] = None):
        assert len(unique_id) == Comm.ID_BYTES
        self.ctx, self.nranks, self.rank = ctx, nranks, rank
        self.lib = ctx.lib if ctx is not None else (lib or load())
        buf = (C.c_ubyte * Comm.ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        self._check(self.lib.dll.lthip_comm_create(self._ctx_h(), nranks, rank, C.addressof(buf), C.byref(h)), "lthip_comm_create")
        self.h = h

    def _ctx_h(self):
        return self.ctx.h if self.ctx is not None else None

    def _check(self, err, what):
        if self.ctx is not None:
            self.ctx._check(err, what)
        elif err:
            raise LongtailHipError(err, what)

    def sync(self):
        if self.ctx is not None:
            self.ctx.sync()

    def info(self) -> dict:
        """Size of the communicator as the TRANSPORT reports it (ncclCommCount), this rank, the transport's name."""
        n, r, t = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.dll.lthip_comm_info(self.h, C.byref(n), C.byref(r), C.byref(t)), "lthip_comm_info")
        return {"nranks": int(n.value), "rank": int(r.value), "transport": Comm.TRANSPORTS.get(int(t.value), str(t.value))}

    def allgather(self, send, recv=None):
        """`send`: contiguous tensor; returns `recv` = the ranks' tensors back to back (nranks * send.numel() elements)."""
        import torch

        send = send.contiguous()
        if recv is None:
            recv = torch.empty(send.numel() * self.nranks, dtype=send.dtype, device=send.device)
        self._check(self.lib.dll.lthip_comm_allgather(self._ctx_h(), self.h, _ptr(send), _ptr(recv), send.numel(), send.element_size()),
                    "lthip_comm_allgather")
        return recv

    def alltoallv(self, send, send_counts, recv_counts, recv=None):
        """`send`: this rank's elements grouped by destination rank (send_counts[p] of them for rank p, back to back); returns the
        elements received, grouped by source rank (recv_counts[p] from rank p).  Counts are host integers."""
        import torch

        send = send.contiguous()
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.uint64)
        assert len(sc) == self.nranks and len(rc) == self.nranks and int(sc.sum()) == send.numel()
        sd = np.zeros(self.nranks, np.uint64)
        rd = np.zeros(self.nranks, np.uint64)
        np.cumsum(sc[:-1], out=sd[1:])
        np.cumsum(rc[:-1], out=rd[1:])
        if recv is None:
            recv = torch.empty(int(rc.sum()), dtype=send.dtype, device=send.device)
        self._check(self.lib.dll.lthip_comm_alltoallv(self._ctx_h(), self.h, _ptr(send) if send.numel() else None, sc.ctypes.data, sd.ctypes.data,
                                                      _ptr(recv) if recv.numel() else None, rc.ctypes.data, rd.ctypes.data, send.element_size()),
                    "lthip_comm_alltoallv")
        return recv

    def close(self):
        if self.h:
            self.lib.dll.lthip_comm_destroy(self.h)
            self.h = None


class IngestConfig(C.Structure):
    _fields_ = [("target_chunk_size", C.c_uint32), ("hash_identifier", C.c_uint32), ("max_block_size", C.c_uint32),
                ("max_chunks_per_block", C.c_uint32), ("compression_type", C.c_uint32), ("codec", C.c_uint32),
                ("batch_bytes", C.c_uint64)]


class IngestTree(C.Structure):
    _fields_ = [("asset_count", C.c_uint32), ("asset_sizes", C.c_void_p), ("path_start_offsets", C.c_void_p),
                ("permissions", C.c_void_p), ("path_data", C.c_char_p), ("path_data_size", C.c_uint32), ("asset_tags", C.c_void_p),
                ("job_count", C.c_uint64), ("job_asset", C.c_void_p), ("job_first", C.c_void_p), ("my_job_count", C.c_uint64),
                ("my_jobs", C.c_void_p)]


class IngestResult(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("struct_size", "chunks_all", "unique_all", "chunks_local", "unique_local", "blocks", "raw_bytes",
                                          "compressed_bytes", "gathered_blocks", "version_index_size", "store_index_size", "gathered_bytes")]


CODECS = {"none": 0, "lz4": 1, "zstd": 2, "by-tag": 3}  # enum lthip_codec; "by-tag": every block's codec follows its own tag
LZ4_TYPE = 0x6C7A3432    # 'lz42', lib/lz4/longtail_lz4.c:10
ZSTD_DEFAULT = 0x7A746432  # 'ztd2', lib/zstd/longtail_zstd.c:12-22 (ZSTD default quality)


def _default_tag(codec: str, compression_type: Optional[int], has_tags: bool) -> int:
    """cfg.compression_type where the caller gave none: the codec's own tag; 0 for "none" (the only tag it writes).  "by-tag" has no
    default: the caller passes compression_type or asset tags (cfg.compression_type is then 0, a tag the mode takes)."""
    if compression_type is not None:
        return compression_type
    if codec == "by-tag":
        if not has_tags:
            raise ValueError('codec "by-tag" needs compression_type or asset tags')
        return 0
    return {"none": 0, "lz4": LZ4_TYPE, "zstd": ZSTD_DEFAULT}[codec]


class Ingest:
    """lthip_ingest: CreateVersionIndex tail + CreateMissingContent + WriteContent over device-resident chunk lists."""

    def __init__(self, ctx: "Context", target_chunk_size: int, max_block_size: int, max_chunks_per_block: int, codec: str,
                 compression_type: Optional[int] = None, batch_bytes: int = 0, hash_identifier: int = 0x626C6B33):
        self.ctx = ctx
        # ("by-tag" without compression_type: the tags come with the tree, index() insists on them)
        self._needs_tags = codec == "by-tag" and compression_type is None
        compression_type = _default_tag(codec, compression_type, True)
        self.cfg = IngestConfig(target_chunk_size, hash_identifier, max_block_size, max_chunks_per_block, compression_type,
                                CODECS[codec], batch_bytes)
        h = C.c_void_p()
        ctx._check(ctx.lib.dll.lthip_ingest_create(ctx.h, C.byref(self.cfg), C.byref(h)), "lthip_ingest_create")
        self.h = h
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dll.lthip_ingest_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def tree(asset_sizes, path_start_offsets, permissions, path_data: bytes, job_asset, job_first, my_jobs=None, asset_tags=None):
        """-> (IngestTree, keep-alive list)."""
        a_sz, a_off = _u64arr(asset_sizes), _u32arr(path_start_offsets)
        a_perm = np.ascontiguousarray(np.asarray(permissions, dtype=np.uint16))
        j_as, j_first = _u32arr(job_asset), _u64arr(job_first)
        mine = _u64arr(my_jobs) if my_jobs is not None else None
        tags = _u32arr(asset_tags) if asset_tags is not None else None
        t = IngestTree(len(a_sz), a_sz.ctypes.data, a_off.ctypes.data, a_perm.ctypes.data, path_data, len(path_data),
                       tags.ctypes.data if tags is not None else None, len(j_as), j_as.ctypes.data, j_first.ctypes.data,
                       len(mine) if mine is not None else 0, mine.ctypes.data if mine is not None else None)
        keep = [a_sz, a_off, a_perm, path_data, j_as, j_first, mine, tags]
        t._keep = keep  # the arrays are read during index() only (the session copies what its helper thread needs later)
        return t, keep

    def index(self, tree: IngestTree, all_hashes, all_lens, all_chunks: int, local_offsets, local_part_first, local_chunks: int,
              version_index_out=None):
        """version_index_out: a (pinned) uint8 torch tensor or numpy array, or None."""
        if getattr(self, "_needs_tags", False) and not tree.asset_tags:
            raise ValueError('codec "by-tag" needs compression_type or asset tags')
        cap = 0 if version_index_out is None else (version_index_out.numel() if hasattr(version_index_out, "numel") else len(version_index_out))
        err = self.ctx.lib.dll.lthip_ingest_index(self.h, C.byref(tree), _ptr(all_hashes), _ptr(all_lens), all_chunks, _ptr(local_offsets),
                                                  _ptr(local_part_first), local_chunks, _ptr(version_index_out) or None, cap)
        self._index_keep = (tree, all_hashes, all_lens, local_offsets, local_part_first, version_index_out)  # until finish()
        self.ctx._check(err, "lthip_ingest_index")

    def set_first_seen(self, first_index, unique_chunks: int):
        """first-seen index of every chunk from the sharded table (longtail_amd.dist.sharded_first_seen): the next index() uses it."""
        self._first_keep = first_index  # must stay alive until index() has returned
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_set_first_seen(self.h, _ptr(first_index), C.c_uint64(int(unique_chunks))),
                        "lthip_ingest_set_first_seen")

    def set_store(self, store: "Optional[Store]"):
        """The following index() calls write only what `store` lacks (None detaches it); the store must outlive them."""
        self._store_keep = store
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_set_store(self.h, store.h if store is not None else None), "lthip_ingest_set_store")

    def store_stats(self):
        """(chunks, bytes) of the first-seen chunks of this rank's jobs that the attached store held; (0, 0) without a store."""
        c, b = C.c_uint64(0), C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_store_stats(self.h, C.byref(c), C.byref(b)), "lthip_ingest_store_stats")
        return int(c.value), int(b.value)

    def write(self, data, arena):
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_write(self.h, _ptr(data), _ptr(arena), int(arena.numel())), "lthip_ingest_write")

    def finish(self, store_index_out=None) -> IngestResult:
        cap = 0 if store_index_out is None else (store_index_out.numel() if hasattr(store_index_out, "numel") else len(store_index_out))
        res = IngestResult()
        res.struct_size = C.sizeof(IngestResult)
        err = self.ctx.lib.dll.lthip_ingest_finish(self.h, _ptr(store_index_out) or None, cap, C.byref(res))
        self.ctx._check(err, "lthip_ingest_finish")
        self._index_keep = None
        return res

    def images(self):
        """(first block, offsets into the arena [u64], image sizes [u32]) of the last codec batch: the stored-block images a host-fed
        embedder downloads (lthip_ingest_images; valid after finish())."""
        first, count, po, ps = C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_void_p()
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_images(self.h, C.byref(first), C.byref(count), C.byref(po), C.byref(ps)), "lthip_ingest_images")
        n = int(count.value)
        if n == 0:
            return int(first.value), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        return (int(first.value), np.ctypeslib.as_array((C.c_uint64 * n).from_address(po.value)).copy(),
                np.ctypeslib.as_array((C.c_uint32 * n).from_address(ps.value)).copy())

    def compressed_sizes(self, nblocks: int) -> np.ndarray:
        p = self.ctx.lib.dll.lthip_ingest_compressed_sizes(self.h)
        if not p or nblocks == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array((C.c_uint32 * nblocks).from_address(p)).copy()


def _numel(buf) -> int:
    return 0 if buf is None else int(buf.numel() if hasattr(buf, "numel") else len(buf))


class Seen:
    """lthip_seen: the first-seen table that is kept between calls and grows -- add() over the pieces of an array gives, concatenated,
    what Context.dedup_first_seen gives for the whole array."""

    def __init__(self, ctx: "Context", expected_hashes: int = 0):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.dll.lthip_seen_create(ctx.h, expected_hashes, C.byref(h)), "lthip_seen_create")
        self.h = h
        self._keep = []

    def close(self):
        # (the C object reads its context when it is destroyed: a table that outlives its context is dropped, not touched again)
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.dll.lthip_seen_destroy(self.h)
        self.h = None
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, hashes):
        """-> (first index of every hash: int32 tensor of positions over everything added so far, distinct hashes in the table: a
        one-element int64 device tensor).  Asynchronous on the context's stream."""
        torch = self.ctx.torch
        n = int(hashes.numel())
        first = torch.empty(max(1, n), dtype=torch.int32, device=self.ctx._dev())
        distinct = torch.zeros(1, dtype=torch.int64, device=self.ctx._dev())
        self.ctx._check(self.ctx.lib.dll.lthip_seen_add(self.h, n, _ptr(hashes) if n else None, _ptr(first), _ptr(distinct)), "lthip_seen_add")
        self._keep.append(hashes)  # read by the launches the call queued: kept until sync() or close()
        return first[:n], distinct

    def find(self, hashes):
        """-> int32 tensor: the position of the first occurrence of every hash among everything added so far, -1 (0xFFFFFFFF) where
        the table does not hold it.  Answers what the add() calls before it put in; asynchronous on the context's stream."""
        torch = self.ctx.torch
        n = int(hashes.numel())
        position = torch.empty(max(1, n), dtype=torch.int32, device=self.ctx._dev())
        self.ctx._check(self.ctx.lib.dll.lthip_seen_find(self.h, n, _ptr(hashes) if n else None, _ptr(position)), "lthip_seen_find")
        self._keep.append(hashes)
        return position[:n]

    def sync(self):
        """Waits for the context's stream; the inputs of the add() calls so far are let go."""
        self.ctx.sync()
        self._keep = []

    @property
    def total(self) -> int:
        return int(self.ctx.lib.dll.lthip_seen_total(self.h))

    @property
    def grown(self) -> int:
        return int(self.ctx.lib.dll.lthip_seen_grown(self.h))


class Store:
    """lthip_store: the set of chunk hashes a store already holds, resident on the device -- built from StoreIndex blobs (add_index) or
    device hashes (add), asked with find(), attached to a session with IngestStream.set_store / Ingest.set_store so that the session
    writes only what the store lacks."""

    def __init__(self, ctx: "Context", expected_hashes: int = 0):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._check(ctx.lib.dll.lthip_store_create(ctx.h, expected_hashes, C.byref(h)), "lthip_store_create")
        self.h = h
        self._keep = []

    def close(self):
        # (the C object reads its context when it is destroyed: a store that outlives its context is dropped, not touched again)
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.dll.lthip_store_destroy(self.h)
        self.h = None
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, hashes):
        """`hashes`: a device int64 / uint64 tensor, duplicates allowed.  Asynchronous on the context's stream."""
        n = int(hashes.numel())
        self.ctx._check(self.ctx.lib.dll.lthip_store_add(self.h, n, _ptr(hashes) if n else None), "lthip_store_add")
        self._keep.append(hashes)  # read by the launch the call queued: kept until sync() or close()

    def add_index(self, store_index: bytes):
        """The chunk hashes of a serialized StoreIndex (host bytes); EBADF for a malformed one, which changes nothing."""
        raw = np.frombuffer(store_index, np.uint8)
        self.ctx._check(self.ctx.lib.dll.lthip_store_add_index(self.h, raw.ctypes.data if len(raw) else None, len(raw)), "lthip_store_add_index")

    def find(self, hashes, count=None):
        """-> (known: uint8 tensor, 1 where the store holds the hash; their number: a one-element int64 device tensor -- `count`, if
        given: the call sets it, it does not add to it)"""
        torch = self.ctx.torch
        n = int(hashes.numel())
        known = torch.empty(max(1, n), dtype=torch.uint8, device=self.ctx._dev())
        if count is None:
            count = torch.full((1,), -1, dtype=torch.int64, device=self.ctx._dev())
        self.ctx._check(self.ctx.lib.dll.lthip_store_find(self.h, n, _ptr(hashes) if n else None, _ptr(known), _ptr(count)), "lthip_store_find")
        self._keep.append(hashes)
        return known[:n], count

    def sync(self):
        """Waits for the context's stream; the inputs of the add() / find() calls so far are let go."""
        self.ctx.sync()
        self._keep = []

    @property
    def added(self) -> int:
        return int(self.ctx.lib.dll.lthip_store_added(self.h))

    @property
    def distinct(self) -> int:
        out = C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_store_distinct(self.h, C.byref(out)), "lthip_store_distinct")
        self._keep = []
        return int(out.value)

    @property
    def grown(self) -> int:
        return int(self.ctx.lib.dll.lthip_store_grown(self.h))


class IngestStream:
    """lthip_ingest_stream: the ingest session for a tree that arrives in slices of jobs -- one first-seen table, one packing and one
    VersionIndex / StoreIndex pair for the whole tree, wherever the slices were cut (include/longtail_hip.h)."""

    def __init__(self, ctx: "Context", tree: IngestTree, target_chunk_size: int, max_block_size: int, max_chunks_per_block: int, codec: str,
                 compression_type: Optional[int] = None, hash_identifier: int = 0x626C6B33):
        self.ctx = ctx
        compression_type = _default_tag(codec, compression_type, bool(tree.asset_tags))
        self.cfg = IngestConfig(target_chunk_size, hash_identifier, max_block_size, max_chunks_per_block, compression_type, CODECS[codec], 0)
        h = C.c_void_p()
        ctx._check(ctx.lib.dll.lthip_ingest_stream_create(ctx.h, C.byref(self.cfg), C.byref(tree), C.byref(h)), "lthip_ingest_stream_create")
        self.h = h
        self._keep = None

    def close(self):
        # (the C object reads its context when it is destroyed: a session that outlives its context is dropped, not touched again)
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.dll.lthip_ingest_stream_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def arena_bound(self, slice_bytes: int, slice_chunks: int) -> int:
        """bytes of arena that hold the images of any slice of that many bytes and chunks (host arithmetic)"""
        return int(self.ctx.lib.dll.lthip_ingest_stream_arena_bound(C.byref(self.cfg), slice_bytes, slice_chunks))

    def slice(self, first_job: int, job_count: int, data, chunk_offsets, chunk_lens, chunk_hashes, part_first, chunks: int, arena):
        """Jobs [first_job, first_job + job_count): `data` and the lists are Context.chunk_hash's of a plan of exactly these jobs."""
        self._keep = (data, chunk_offsets, chunk_lens, chunk_hashes, part_first, arena)  # until the call's work has run
        err = self.ctx.lib.dll.lthip_ingest_stream_slice(self.h, first_job, job_count, _ptr(data), _ptr(chunk_offsets), _ptr(chunk_lens),
                                                         _ptr(chunk_hashes), _ptr(part_first), chunks, _ptr(arena), _numel(arena))
        self.ctx._check(err, "lthip_ingest_stream_slice")

    def images(self):
        """(first block, offsets into the arena [u64], image sizes [u32]) of the LAST slice() or finish() call; waits for that call's
        work, after which the caller's data, lists and (once the images are read) arena are its own again."""
        first, count, po, ps = C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_void_p()
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_stream_images(self.h, C.byref(first), C.byref(count), C.byref(po), C.byref(ps)),
                        "lthip_ingest_stream_images")
        self._keep = None
        n = int(count.value)
        if n == 0:
            return int(first.value), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
        return (int(first.value), np.ctypeslib.as_array((C.c_uint64 * n).from_address(po.value)).copy(),
                np.ctypeslib.as_array((C.c_uint32 * n).from_address(ps.value)).copy())

    def finish(self, arena, version_index_out=None, store_index_out=None) -> IngestResult:
        """Closes the open block into `arena` and serializes both indexes of the whole tree into the (pinned) uint8 buffers.  A buffer
        that is too small raises ENOMEM; `last_result` then holds both sizes and the call may be repeated."""
        res = IngestResult()
        res.struct_size = C.sizeof(IngestResult)
        self.last_result = res
        err = self.ctx.lib.dll.lthip_ingest_stream_finish(self.h, _ptr(arena), _numel(arena), _ptr(version_index_out) or None,
                                                          _numel(version_index_out), _ptr(store_index_out) or None, _numel(store_index_out),
                                                          C.byref(res))
        self.ctx._check(err, "lthip_ingest_stream_finish")
        return res

    @property
    def table_grown(self) -> int:
        return int(self.ctx.lib.dll.lthip_ingest_stream_table_grown(self.h))

    def set_store(self, store: "Optional[Store]"):
        """Before the first slice(): the session writes only what `store` lacks (None detaches it); the store must outlive it."""
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_stream_set_store(self.h, store.h if store is not None else None),
                        "lthip_ingest_stream_set_store")
        self._store_keep = store

    def store_stats(self):
        """(chunks, bytes) of the version-unique chunks so far that the attached store held; (0, 0) without a store."""
        c, b = C.c_uint64(0), C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_ingest_stream_store_stats(self.h, C.byref(c), C.byref(b)), "lthip_ingest_stream_store_stats")
        return int(c.value), int(b.value)


class RestoreConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("verify", C.c_uint32)]


class RestoreResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint64)] + [(n, C.c_uint64) for n in (
        "assets_selected", "occurrences", "occurrences_written", "bytes_written", "blocks_needed", "blocks_delivered", "blocks_unneeded",
        "blocks_bad", "chunks_mismatched", "decoded_bytes", "base_occurrences", "base_bytes", "base_chunks_mismatched")]


class RestoreBase(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("version_index", C.c_void_p), ("version_index_size", C.c_uint64), ("asset_offsets", C.c_void_p),
                ("base_bytes", C.c_uint64)]


class RestoreWindow(C.Structure):
    """lthip_restore_window: bytes [offset, offset + length) of asset `asset`, written at `dst` of the output."""
    _fields_ = [("asset", C.c_uint32), ("reserved", C.c_uint32), ("offset", C.c_uint64), ("length", C.c_uint64), ("dst", C.c_uint64)]


RESTORE_WINDOW_DTYPE = np.dtype([("asset", "<u4"), ("reserved", "<u4"), ("offset", "<u8"), ("length", "<u8"), ("dst", "<u8")])


def _window_table(windows) -> np.ndarray:
    """(n, 4) uint64 rows of (asset, offset, length, dst), or a sequence of such tuples -> the lthip_restore_window array."""
    rows = np.asarray(windows if len(windows) else np.zeros((0, 4)), dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[1] != 4:
        raise ValueError("windows: (n, 4) rows of (asset, offset, length, dst)")
    if len(rows) and int(rows[:, 0].max()) > 0xFFFFFFFF:
        raise ValueError("windows: an asset index above 32 bits")
    table = np.zeros(len(rows), RESTORE_WINDOW_DTYPE)
    table["asset"], table["offset"], table["length"], table["dst"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    return table


RESTORE_SKIP = 0xFFFFFFFFFFFFFFFF  # include/longtail_hip.h LTHIP_RESTORE_SKIP
RESTORE_NOT_DELIVERED, RESTORE_BAD_HEADER, RESTORE_BAD_PAYLOAD, RESTORE_BAD_CHUNK = 1, 2, 4, 8


class Restore:
    """lthip_restore: stored-block images in HBM back into a version's assets, asset a at asset_offsets[a] of one device buffer
    (include/longtail_hip.h, "the restore session").  layout() -> offsets; needed_blocks() -> which blocks to fetch; blocks() per batch of
    images; finish() -> (0 / ENOENT: blocks outstanding / EBADF: a bad block, the result).

    base = (version_index, asset_offsets, base_bytes) of a version that lies restored in device memory: the chunks it shares with the
    target are planned as copies from it (carry(base_tensor, out), in any order with blocks()), needed_blocks() shrinks to the blocks that
    hold a chunk no resident asset has, and store_index may be the small one an incremental ingest returned.

    windows = (n, 4) uint64 rows of (asset, offset, length, dst), with asset_offsets None: the session restores byte windows of assets
    (lthip_restore_create_windows) -- part of a file, or a rank's share from restore_rank_windows.  No base with windows."""

    SKIP = RESTORE_SKIP

    @staticmethod
    def layout(version_index: bytes, align: int = 1, lib: Optional[HipLib] = None):
        """-> (asset offsets: uint64 array, total bytes) of the dense layout at `align`-byte boundaries; host only."""
        dll = (lib or load()).dll
        raw = np.frombuffer(version_index, np.uint8)
        n, total = C.c_uint32(0), C.c_uint64(0)
        err = dll.lthip_restore_layout(raw.ctypes.data if len(raw) else None, len(raw), align, None, C.byref(n), C.byref(total))
        if err:
            raise LongtailHipError(err, "lthip_restore_layout")
        offsets = np.zeros(n.value, np.uint64)
        err = dll.lthip_restore_layout(raw.ctypes.data, len(raw), align, offsets.ctypes.data, C.byref(n), C.byref(total))
        if err:
            raise LongtailHipError(err, "lthip_restore_layout")
        return offsets, int(total.value)

    def __init__(self, ctx: "Context", version_index: bytes, store_index: bytes, asset_offsets, out_bytes: int, verify: bool = True, base=None,
                 windows=None):
        self.ctx = ctx
        self.h = None
        if windows is not None and asset_offsets is not None:
            raise ValueError("give asset_offsets or windows, not both")
        if windows is not None and base is not None:
            raise ValueError("a window session has no base")
        vi, si = np.frombuffer(version_index, np.uint8), np.frombuffer(store_index, np.uint8)
        cfg = RestoreConfig(C.sizeof(RestoreConfig), 1 if verify else 0)
        h = C.c_void_p()
        if windows is not None:
            table = _window_table(windows)
            ctx._check(ctx.lib.dll.lthip_restore_create_windows(ctx.h, C.byref(cfg), vi.ctypes.data if len(vi) else None, len(vi),
                                                                si.ctypes.data if len(si) else None, len(si), len(table),
                                                                table.ctypes.data if len(table) else None, out_bytes, C.byref(h)),
                       "lthip_restore_create_windows")
            self.h = h
            self._keep = []
            return
        offs = _u64arr(asset_offsets)
        args = (vi.ctypes.data if len(vi) else None, len(vi), si.ctypes.data if len(si) else None, len(si),
                offs.ctypes.data if len(offs) else None, out_bytes, C.byref(h))
        if base is None:
            ctx._check(ctx.lib.dll.lthip_restore_create(ctx.h, C.byref(cfg), *args), "lthip_restore_create")
        else:
            bvi, boffs = np.frombuffer(base[0], np.uint8), _u64arr(base[1])
            desc = RestoreBase(C.sizeof(RestoreBase), bvi.ctypes.data if len(bvi) else None, len(bvi), boffs.ctypes.data if len(boffs) else None,
                               int(base[2]))
            ctx._check(ctx.lib.dll.lthip_restore_create_from_base(ctx.h, C.byref(cfg), C.byref(desc), *args), "lthip_restore_create_from_base")
        self.h = h
        self._keep = []

    def close(self):
        # (the C object reads its context when it is destroyed: a session that outlives its context is dropped, not touched again)
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.dll.lthip_restore_destroy(self.h)
        self.h = None
        self._keep = []
        self._cache = None  # (the session is gone: the cache it was attached to may go too)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def needed_blocks(self) -> np.ndarray:
        """The hashes of the blocks that hold a chunk of a selected asset, in StoreIndex order."""
        n = C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_needed_blocks(self.h, None, 0, C.byref(n)), "lthip_restore_needed_blocks")
        out = np.zeros(n.value, np.uint64)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_needed_blocks(self.h, out.ctypes.data, len(out), C.byref(n)), "lthip_restore_needed_blocks")
        return out

    def scratch_bound(self, block_hashes) -> int:
        h = _u64arr(block_hashes)
        return int(self.ctx.lib.dll.lthip_restore_scratch_bound(self.h, len(h), h.ctypes.data if len(h) else None))

    def blocks(self, block_hashes, images, image_offsets, image_sizes, scratch, out):
        """Delivers the images (a device uint8 tensor; image i at image_offsets[i], image_sizes[i] bytes) of these blocks; `scratch`: a
        device uint8 tensor of at least scratch_bound(block_hashes) bytes, or None.  Asynchronous on the context's stream: the tensors
        are kept until finish() or close()."""
        h, o, z = _u64arr(block_hashes), _u64arr(image_offsets), _u32arr(image_sizes)
        assert len(h) == len(o) == len(z)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_blocks(self.h, len(h), h.ctypes.data if len(h) else None, _ptr(images),
                                                              o.ctypes.data if len(o) else None, z.ctypes.data if len(z) else None,
                                                              _ptr(scratch), _numel(scratch), _ptr(out)), "lthip_restore_blocks")
        self._keep.append((images, scratch, out))

    def carry(self, base_tensor, out):
        """Queues the copy of every occurrence the base feeds from `base_tensor` (the device uint8 tensor the base's asset offsets refer
        to) into `out`; once per session, in any order with blocks().  Asynchronous on the context's stream: the tensors are kept until
        finish() or close()."""
        self.ctx._check(self.ctx.lib.dll.lthip_restore_carry(self.h, _ptr(base_tensor) or None, _ptr(out) or None), "lthip_restore_carry")
        self._keep.append((base_tensor, out))

    def in_place_scratch_bound(self) -> int:
        """Bytes of scratch carry_in_place needs: moved bytes + 16 x moved occurrences + 64, or 0 when nothing moves."""
        return int(self.ctx.lib.dll.lthip_restore_in_place_scratch_bound(self.h))

    def in_place_stats(self):
        """-> (kept occurrences, kept bytes, moved occurrences, moved bytes) of what the base feeds, when base and target share a buffer."""
        out = np.zeros(4, np.uint64)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_in_place_stats(self.h, out.ctypes.data), "lthip_restore_in_place_stats")
        return tuple(int(x) for x in out)

    def carry_in_place(self, buf, scratch):
        """Queues the update in place: `buf` (a device uint8 tensor of max(base bytes, out bytes)) holds the base and becomes the target;
        what moves goes through `scratch` (at least in_place_scratch_bound() bytes; None when nothing moves), all reads before all writes.
        Once per session and before the first blocks() call, whose `out` is then `buf`.  Asynchronous on the context's stream."""
        self.ctx._check(self.ctx.lib.dll.lthip_restore_carry_in_place(self.h, _ptr(buf) or None, _ptr(scratch) or None, _numel(scratch)),
                        "lthip_restore_carry_in_place")
        self._keep.append((buf, scratch))

    def set_cache(self, cache: "BlockCache"):
        """Attaches a BlockCache of the same context, once and before the first blocks() call: needed_blocks() shrinks to the blocks the
        cache does not feed, good delivered blocks stay in the cache.  The cache object is kept alive while the session is."""
        self.ctx._check(self.ctx.lib.dll.lthip_restore_set_cache(self.h, cache.h if cache is not None else None), "lthip_restore_set_cache")
        self._cache = cache

    def from_cache(self, out):
        """Queues the scatter of the cache-fed blocks from their slots into `out`; once per session, in any order with blocks()."""
        self.ctx._check(self.ctx.lib.dll.lthip_restore_from_cache(self.h, _ptr(out) or None), "lthip_restore_from_cache")
        self._keep.append((out,))

    def cache_stats(self):
        """-> (cache-fed blocks, their raw bytes, blocks inserted, blocks bypassed, blocks dropped as bad, cache-fed entries scattered)."""
        out = np.zeros(6, np.uint64)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_cache_stats(self.h, out.ctypes.data), "lthip_restore_cache_stats")
        return tuple(int(x) for x in out)

    def archive_blocks(self, archive: "Archive", window, window_first_byte: int, scratch, out, window_bytes: Optional[int] = None):
        """Delivers every needed, not yet delivered block of `archive` that lies wholly inside body bytes [window_first_byte,
        + window_bytes), which lie at `window` (a device uint8 tensor; window_bytes defaults to its length), at whatever byte position.
        `scratch`: at least archive_scratch_bound(archive, window_first_byte, window_bytes) bytes, or None.  -> (blocks delivered, the
        lowest body offset of a needed block still outstanding, or the body's size).  Asynchronous like blocks()."""
        n = _numel(window) if window_bytes is None else int(window_bytes)
        delivered, next_byte = C.c_uint32(0), C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_archive_blocks(self.h, archive.h, _ptr(window) or None, window_first_byte, n,
                                                                      _ptr(scratch) or None, _numel(scratch), _ptr(out) or None,
                                                                      C.byref(delivered), C.byref(next_byte)), "lthip_restore_archive_blocks")
        self._keep.append((window, scratch, out))
        return int(delivered.value), int(next_byte.value)

    def archive_scratch_bound(self, archive: "Archive", window_first_byte: int, window_bytes: int) -> int:
        return int(self.ctx.lib.dll.lthip_restore_archive_scratch_bound(self.h, archive.h, window_first_byte, window_bytes))

    def archive_ranges(self, archive: "Archive", max_gap: int = 0) -> np.ndarray:
        """-> (n, 2) uint64 rows of (first body byte, bytes): the needed, outstanding blocks' ranges, sorted, merged where the gap between
        two is at most max_gap; host only."""
        n = C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_archive_ranges(self.h, archive.h, max_gap, None, 0, C.byref(n)), "lthip_restore_archive_ranges")
        out = np.zeros((n.value, 2), np.uint64)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_archive_ranges(self.h, archive.h, max_gap, out.ctypes.data if len(out) else None, len(out),
                                                                      C.byref(n)), "lthip_restore_archive_ranges")
        return out

    def finish(self):
        """-> (code, RestoreResult): 0, errno.ENOENT (needed blocks are outstanding, or the base has not been carried: deliver / carry
        and call again) or errno.EBADF (a delivered block was bad, or with verify a chunk of the base).  The session's one full
        synchronisation."""
        res = RestoreResult()
        res.struct_size = C.sizeof(RestoreResult)
        code = self.ctx.lib.dll.lthip_restore_finish(self.h, C.byref(res))
        if code not in (0, errno.ENOENT, errno.EBADF):
            self.ctx._check(code, "lthip_restore_finish")
        self._keep = []
        return code, res

    def block_status(self, block_hashes) -> np.ndarray:
        """After finish(): per block 0 or RESTORE_* flag bits."""
        h = _u64arr(block_hashes)
        out = np.zeros(len(h), np.uint32)
        self.ctx._check(self.ctx.lib.dll.lthip_restore_block_status(self.h, len(h), h.ctypes.data if len(h) else None,
                                                                    out.ctypes.data if len(h) else None), "lthip_restore_block_status")
        return out


class RepackConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("min_block_usage_percent", C.c_uint32), ("max_block_size", C.c_uint32),
                ("max_chunks_per_block", C.c_uint32), ("verify", C.c_uint32)]


class RepackInfo(C.Structure):
    _fields_ = [("struct_size", C.c_uint64)] + [(n, C.c_uint64) for n in (
        "blocks_total", "blocks_kept", "blocks_dropped", "blocks_source", "live_chunks", "moved_chunks", "moved_bytes", "new_blocks",
        "staging_bytes", "work_bytes", "kept_index_size", "new_index_size", "store_index_size")]


class RepackResult(C.Structure):
    _fields_ = [("struct_size", C.c_uint64)] + [(n, C.c_uint64) for n in (
        "blocks_source", "blocks_delivered", "blocks_bad", "chunks_mismatched", "raw_bytes_written", "compressed_bytes_written",
        "decoded_bytes")]


class Repack:
    """lthip_repack: the live chunks of a store's under-used blocks into new stored-block images (include/longtail_hip.h, "the repack
    session").  live_hashes: a device uint64 tensor (or None for an empty live set).  info() -> the plan; source_blocks() -> which blocks
    to fetch; blocks() per batch of images, all with the same `work` tensor of info().work_bytes; write(work); finish() -> (code, new
    index or None, RepackResult); then images() and store_index().  Delete dropped_blocks() only after finish() returned 0 and the new
    images are stored."""

    def __init__(self, ctx: "Context", store_index: bytes, live_hashes, min_block_usage_percent: int, max_block_size: int,
                 max_chunks_per_block: int, verify: bool = True):
        self.ctx = ctx
        self.h = None
        si = np.frombuffer(store_index, np.uint8)
        n = _numel(live_hashes) if live_hashes is not None else 0
        cfg = RepackConfig(C.sizeof(RepackConfig), min_block_usage_percent, max_block_size, max_chunks_per_block, 1 if verify else 0)
        h = C.c_void_p()
        ctx._check(ctx.lib.dll.lthip_repack_create(ctx.h, C.byref(cfg), si.ctypes.data if len(si) else None, len(si), n,
                                                   _ptr(live_hashes) if n else None, C.byref(h)), "lthip_repack_create")
        self.h = h
        self._keep = []

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.dll.lthip_repack_destroy(self.h)
        self.h = None
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> RepackInfo:
        out = RepackInfo()
        out.struct_size = C.sizeof(RepackInfo)
        self.ctx._check(self.ctx.lib.dll.lthip_repack_plan_info(self.h, C.byref(out)), "lthip_repack_plan_info")
        return out

    def _hashes(self, which: str) -> np.ndarray:
        fn, n = getattr(self.ctx.lib.dll, f"lthip_repack_{which}_blocks"), C.c_uint64(0)
        self.ctx._check(fn(self.h, None, 0, C.byref(n)), f"lthip_repack_{which}_blocks")
        out = np.zeros(n.value, np.uint64)
        self.ctx._check(fn(self.h, out.ctypes.data if len(out) else None, len(out), C.byref(n)), f"lthip_repack_{which}_blocks")
        return out

    def kept_blocks(self) -> np.ndarray:
        """The hashes of the blocks that stay, in the order lthip_get_existing_store_index lists them."""
        return self._hashes("kept")

    def dropped_blocks(self) -> np.ndarray:
        """The hashes of the blocks that do not stay, in StoreIndex order."""
        return self._hashes("dropped")

    def source_blocks(self) -> np.ndarray:
        """The hashes of the blocks a moved chunk comes from, in StoreIndex order: the ones to deliver."""
        return self._hashes("source")

    def kept_index(self) -> bytes:
        """The serialized StoreIndex of the kept blocks: byte for byte lthip_get_existing_store_index's."""
        return _sized_blob_call(self.ctx.lib.dll.lthip_repack_kept_index, "lthip_repack_kept_index", self.h)

    def scratch_bound(self, block_hashes) -> int:
        h = _u64arr(block_hashes)
        return int(self.ctx.lib.dll.lthip_repack_scratch_bound(self.h, len(h), h.ctypes.data if len(h) else None))

    def blocks(self, block_hashes, images, image_offsets, image_sizes, scratch, work):
        """Delivers the images of these blocks, as Restore.blocks does, with the work buffer as the output.  Asynchronous on the
        context's stream: the tensors are kept until finish() or close()."""
        h, o, z = _u64arr(block_hashes), _u64arr(image_offsets), _u32arr(image_sizes)
        assert len(h) == len(o) == len(z)
        self.ctx._check(self.ctx.lib.dll.lthip_repack_blocks(self.h, len(h), h.ctypes.data if len(h) else None, _ptr(images),
                                                             o.ctypes.data if len(o) else None, z.ctypes.data if len(z) else None,
                                                             _ptr(scratch), _numel(scratch), _ptr(work)), "lthip_repack_blocks")
        self._keep.append((images, scratch, work))

    def write(self, work):
        """Queues the block writer for all new blocks; ENOENT (raised) while source blocks are outstanding."""
        self.ctx._check(self.ctx.lib.dll.lthip_repack_write(self.h, _ptr(work) or None, _numel(work)), "lthip_repack_write")
        self._keep.append((work,))

    def finish(self):
        """-> (code, the new index's bytes or None, RepackResult): 0, errno.ENOENT (source blocks or write() are outstanding) or
        errno.EBADF (a delivered block was bad: delete nothing).  The session's one full synchronisation."""
        res = RepackResult()
        res.struct_size = C.sizeof(RepackResult)
        n = C.c_size_t(self.info().new_index_size)
        out = np.zeros(max(n.value, 1), np.uint8)
        code = self.ctx.lib.dll.lthip_repack_finish(self.h, out.ctypes.data, n.value, C.byref(n), C.byref(res))
        if code not in (0, errno.ENOENT, errno.EBADF):
            self.ctx._check(code, "lthip_repack_finish")
        self._keep = []
        return code, (out[: n.value].tobytes() if code == 0 else None), res

    def images(self):
        """After finish() returned 0 -> (offsets: uint64 array, sizes: uint32 array): image i of the new index lies at work[offsets[i]:]."""
        n, po, pz = C.c_uint64(0), C.c_void_p(), C.c_void_p()
        self.ctx._check(self.ctx.lib.dll.lthip_repack_images(self.h, C.byref(n), C.byref(po), C.byref(pz)), "lthip_repack_images")
        k = n.value
        offs = np.frombuffer(C.string_at(po.value, 8 * k), np.uint64).copy() if k else np.zeros(0, np.uint64)
        sizes = np.frombuffer(C.string_at(pz.value, 4 * k), np.uint32).copy() if k else np.zeros(0, np.uint32)
        return offs, sizes

    def store_index(self) -> bytes:
        """After finish() returned 0: the store's index afterwards -- the kept blocks (under their own tags), then the new blocks."""
        n = C.c_size_t(0)
        err = self.ctx.lib.dll.lthip_repack_store_index(self.h, None, 0, C.byref(n))
        if err != errno.ENOMEM:
            self.ctx._check(err or errno.EIO, "lthip_repack_store_index")
        out = np.zeros(n.value, np.uint8)
        self.ctx._check(self.ctx.lib.dll.lthip_repack_store_index(self.h, out.ctypes.data, len(out), C.byref(n)), "lthip_repack_store_index")
        return out.tobytes()

    def block_status(self, block_hashes) -> np.ndarray:
        """After finish(): per block 0 or RESTORE_* flag bits."""
        h = _u64arr(block_hashes)
        out = np.zeros(len(h), np.uint32)
        self.ctx._check(self.ctx.lib.dll.lthip_repack_block_status(self.h, len(h), h.ctypes.data if len(h) else None,
                                                                   out.ctypes.data if len(h) else None), "lthip_repack_block_status")
        return out


BLOCK_CACHE_STATS = ("slots", "slot_bytes", "resident", "pinned", "reserved", "hits", "inserted", "evicted", "bypassed", "dropped")


class BlockCache:
    """lthip_block_cache: slot_count device slots of slot_bytes (rounded up to 64) that keep decoded blocks between the Restore sessions
    of one context (include/longtail_hip.h, "a cache of decoded blocks").  Size the slots by the largest raw size among the StoreIndex's blocks (about
    the store's max_block_size): a block larger than a slot is never cached.  Close it after every session attached to it and before the context."""

    def __init__(self, ctx: "Context", slot_count: int, slot_bytes: int):
        self.ctx = ctx
        self.h = None
        h = C.c_void_p()
        ctx._check(ctx.lib.dll.lthip_block_cache_create(ctx.h, slot_count, slot_bytes, C.byref(h)), "lthip_block_cache_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.dll.lthip_block_cache_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def contains(self, hash_identifier: int, block_hashes) -> np.ndarray:
        """Per block hash 1 when the cache holds a visible entry of it under `hash_identifier`, else 0; host only."""
        h = _u64arr(block_hashes)
        held = np.zeros(len(h), np.uint8)
        self.ctx._check(self.ctx.lib.dll.lthip_block_cache_contains(self.h, hash_identifier, len(h), h.ctypes.data if len(h) else None,
                                                                    held.ctypes.data if len(h) else None), "lthip_block_cache_contains")
        return held

    def stats(self) -> dict:
        """-> dict of BLOCK_CACHE_STATS: the state now (slots .. reserved) and the sums since create (hits .. dropped)."""
        out = np.zeros(10, np.uint64)
        self.ctx._check(self.ctx.lib.dll.lthip_block_cache_stats(self.h, out.ctypes.data), "lthip_block_cache_stats")
        return {k: int(v) for k, v in zip(BLOCK_CACHE_STATS, out)}

    def clear(self):
        """Drops every entry; LongtailHipError(EBUSY) while a live session pins an entry or has reserved a slot."""
        self.ctx._check(self.ctx.lib.dll.lthip_block_cache_clear(self.h), "lthip_block_cache_clear")


ARCHIVE_BODY_UNKNOWN = 0xFFFFFFFFFFFFFFFF


def _blob(b):
    raw = np.frombuffer(b, np.uint8)
    return raw, (raw.ctypes.data if len(raw) else None)


def archive_index_size(store_index: bytes, version_index: bytes, lib: Optional[HipLib] = None) -> int:
    """lthip_archive_index_size, host only: the bytes of the archive index of these two blobs."""
    (si, psi), (vi, pvi) = _blob(store_index), _blob(version_index)
    n = C.c_uint64(0)
    err = (lib or load()).dll.lthip_archive_index_size(psi, len(si), pvi, len(vi), C.byref(n))
    if err:
        raise LongtailHipError(err, "lthip_archive_index_size")
    return int(n.value)


def archive_write_index(store_index: bytes, version_index: bytes, block_offsets, block_sizes, lib: Optional[HipLib] = None) -> bytes:
    """lthip_archive_write_index, host only: the archive index with block b at body offset block_offsets[b], block_sizes[b] bytes long."""
    (si, psi), (vi, pvi) = _blob(store_index), _blob(version_index)
    o, z = _u64arr(block_offsets), _u32arr(block_sizes)
    assert len(o) == len(z)
    out = np.full(archive_index_size(store_index, version_index, lib), 0xEE, np.uint8)
    err = (lib or load()).dll.lthip_archive_write_index(psi, len(si), pvi, len(vi), o.ctypes.data if len(o) else None,
                                                        z.ctypes.data if len(z) else None, out.ctypes.data, len(out))
    if err:
        raise LongtailHipError(err, "lthip_archive_write_index")
    return out.tobytes()


def archive_peek(first_8_bytes: bytes, lib: Optional[HipLib] = None) -> int:
    """lthip_archive_peek: the first eight bytes of an archive -> the bytes of its index."""
    raw = np.frombuffer(first_8_bytes[:8], np.uint8)
    if len(raw) < 8:
        raise LongtailHipError(errno.EBADF, "lthip_archive_peek")
    n = C.c_uint64(0)
    err = (lib or load()).dll.lthip_archive_peek(raw.ctypes.data, C.byref(n))
    if err:
        raise LongtailHipError(err, "lthip_archive_peek")
    return int(n.value)


class Archive:
    """lthip_archive: the opened index of a one-file archive (include/longtail_hip.h, "one-file archives"); host only, no context.
    `index`: the index's bytes (archive_peek says how many); body_bytes: the size of what follows it in the file, None when unknown."""

    def __init__(self, index: bytes, body_bytes: Optional[int] = None, lib: Optional[HipLib] = None):
        self.lib = lib or load()
        self.h = None
        raw, p = _blob(index)
        h = C.c_void_p()
        none = np.zeros(8, np.uint8)  # (no bytes at all are a short index: EBADF, not the EINVAL of a null pointer)
        err = self.lib.dll.lthip_archive_open(p or none.ctypes.data, len(raw), ARCHIVE_BODY_UNKNOWN if body_bytes is None else body_bytes, C.byref(h))
        if err:
            raise LongtailHipError(err, "lthip_archive_open")
        self.h = h
        dll, n = self.lib.dll, C.c_size_t(0)
        p = dll.lthip_archive_store_index(h, C.byref(n))
        self.store_index = C.string_at(p, n.value)
        p = dll.lthip_archive_version_index(h, C.byref(n))
        self.version_index = C.string_at(p, n.value)  # (the rest of the index: up to 7 pad bytes behind the name data)
        self.block_count = int(dll.lthip_archive_block_count(h))
        nb = self.block_count
        self.block_offsets = np.ctypeslib.as_array((C.c_uint64 * nb).from_address(dll.lthip_archive_block_offsets(h))).copy() if nb else np.zeros(0, np.uint64)
        self.block_sizes = np.ctypeslib.as_array((C.c_uint32 * nb).from_address(dll.lthip_archive_block_sizes(h))).copy() if nb else np.zeros(0, np.uint32)
        self.body_bytes = int(dll.lthip_archive_body_bytes(h))
        self.index_bytes = len(raw)

    def close(self):
        if getattr(self, "h", None):
            self.lib.dll.lthip_archive_close(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ArchiveWriter:
    """lthip_archive_writer: packs the images an ingest session left in its arena into the body of a one-file archive, call by call, and
    writes the index from what it recorded (include/longtail_hip.h, "one-file archives")."""

    def __init__(self, ctx: "Context"):
        self.ctx = ctx
        self.h = None
        h = C.c_void_p()
        ctx._check(ctx.lib.dll.lthip_archive_writer_create(ctx.h, C.byref(h)), "lthip_archive_writer_create")
        self.h = h
        self._keep = []

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dll.lthip_archive_writer_destroy(self.h)
        self.h = None
        self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, arena, image_offsets, image_sizes, dst, dst_capacity: Optional[int] = None) -> int:
        """Queues the copy of the images (image i at arena[image_offsets[i]], image_sizes[i] bytes, as IngestStream.images() returns them)
        densely to dst[0:]; -> the bytes written.  The archive's body is the concatenation of all calls' outputs: drain `dst` (after
        Context.sync(), or behind it on the stream) before it is reused."""
        o, z = _u64arr(image_offsets), _u32arr(image_sizes)
        assert len(o) == len(z)
        n = C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_archive_writer_append(self.h, _ptr(arena) or None, len(o), o.ctypes.data if len(o) else None,
                                                                     z.ctypes.data if len(z) else None, _ptr(dst) or None,
                                                                     _numel(dst) if dst_capacity is None else dst_capacity, C.byref(n)),
                        "lthip_archive_writer_append")
        self._keep = [(arena, dst)]
        return int(n.value)

    def blocks(self):
        """-> (body offsets [u64], sizes [u32]) of every block appended so far, and the body's size."""
        n, po, ps, body = C.c_uint64(0), C.c_void_p(), C.c_void_p(), C.c_uint64(0)
        self.ctx._check(self.ctx.lib.dll.lthip_archive_writer_blocks(self.h, C.byref(n), C.byref(po), C.byref(ps), C.byref(body)),
                        "lthip_archive_writer_blocks")
        k = int(n.value)
        if not k:
            return np.zeros(0, np.uint64), np.zeros(0, np.uint32), int(body.value)
        return (np.ctypeslib.as_array((C.c_uint64 * k).from_address(po.value)).copy(),
                np.ctypeslib.as_array((C.c_uint32 * k).from_address(ps.value)).copy(), int(body.value))

    def finish(self, store_index: bytes, version_index: bytes) -> bytes:
        """-> the archive index of the two blobs with the recorded block offsets and sizes."""
        (si, psi), (vi, pvi) = _blob(store_index), _blob(version_index)
        n = C.c_uint64(0)
        err = self.ctx.lib.dll.lthip_archive_writer_finish(self.h, psi, len(si), pvi, len(vi), None, 0, C.byref(n))
        if err != errno.ENOMEM:
            self.ctx._check(err or errno.EIO, "lthip_archive_writer_finish")
        out = np.zeros(n.value, np.uint8)
        self.ctx._check(self.ctx.lib.dll.lthip_archive_writer_finish(self.h, psi, len(si), pvi, len(vi), out.ctypes.data, len(out), C.byref(n)),
                        "lthip_archive_writer_finish")
        return out.tobytes()


def _sized_blob_call(fn, name: str, *args) -> bytes:
    """A host call that ends in (out, capacity, *size): asked for the size (ENOMEM with the size set), then for the bytes."""
    n = C.c_size_t(0)
    err = fn(*args, None, 0, C.byref(n))
    if err != errno.ENOMEM:
        raise LongtailHipError(err, name)
    out = np.full(n.value, 0xEE, np.uint8)
    err = fn(*args, out.ctypes.data, len(out), C.byref(n))
    if err:
        raise LongtailHipError(err, name)
    return out[: n.value].tobytes()


def store_index_prune(store_index: bytes, keep_block_hashes, lib: Optional[HipLib] = None) -> bytes:
    """lthip_store_index_prune, host only: the StoreIndex of the blocks of `store_index` whose hash is among keep_block_hashes, in its
    order (Longtail_PruneStoreIndex, serialized)."""
    (si, psi), keep = _blob(store_index), _u64arr(keep_block_hashes)
    return _sized_blob_call((lib or load()).dll.lthip_store_index_prune, "lthip_store_index_prune", psi, len(si), len(keep),
                            keep.ctypes.data if len(keep) else None)


def store_index_merge(local: bytes, remote: bytes, lib: Optional[HipLib] = None) -> bytes:
    """lthip_store_index_merge, host only: local's blocks, then remote's blocks that local does not hold (Longtail_MergeStoreIndex,
    serialized)."""
    (a, pa), (b, pb) = _blob(local), _blob(remote)
    return _sized_blob_call((lib or load()).dll.lthip_store_index_merge, "lthip_store_index_merge", pa, len(a), pb, len(b))


def version_chunk_hashes(version_index: bytes, lib: Optional[HipLib] = None) -> np.ndarray:
    """lthip_version_chunk_hashes, host only: the chunk hashes of a serialized VersionIndex, in its order (uint64 array)."""
    dll = (lib or load()).dll
    raw, p = _blob(version_index)
    n = C.c_uint64(0)
    err = dll.lthip_version_chunk_hashes(p, len(raw), None, 0, C.byref(n))
    if err not in (0, errno.ENOMEM):
        raise LongtailHipError(err, "lthip_version_chunk_hashes")
    out = np.zeros(n.value, np.uint64)
    err = dll.lthip_version_chunk_hashes(p, len(raw), out.ctypes.data if len(out) else None, len(out), C.byref(n))
    if err:
        raise LongtailHipError(err, "lthip_version_chunk_hashes")
    return out


def version_diff(source_vi: bytes, target_vi: bytes, lib: Optional[HipLib] = None):
    """lthip_version_diff, host only: what changed between two serialized VersionIndexes, the lists of Longtail_CreateVersionDiff ->
    (source_removed, target_added, source_content_modified, target_content_modified, source_permissions_modified,
    target_permissions_modified): uint32 arrays of asset indices."""
    dll = (lib or load()).dll
    a, b = np.frombuffer(source_vi, np.uint8), np.frombuffer(target_vi, np.uint8)
    args = (a.ctypes.data if len(a) else None, len(a), b.ctypes.data if len(b) else None, len(b))
    counts = np.zeros(4, np.uint32)
    err = dll.lthip_version_diff(*args, None, None, None, None, None, None, counts.ctypes.data)
    if err:
        raise LongtailHipError(err, "lthip_version_diff")
    lists = [np.zeros(max(1, int(counts[k])), np.uint32) for k in (0, 1, 2, 2, 3, 3)]
    err = dll.lthip_version_diff(*args, *[x.ctypes.data for x in lists], counts.ctypes.data)
    if err:
        raise LongtailHipError(err, "lthip_version_diff")
    return tuple(x[: int(counts[k])] for x, k in zip(lists, (0, 1, 2, 2, 3, 3)))


def restore_asset_sizes(version_index: bytes, lib: Optional[HipLib] = None):
    """lthip_restore_asset_sizes, host only -> (asset sizes: uint64 array, target chunk size) of a serialized VersionIndex: what
    lthip_make_jobs and lthip_partition_jobs want."""
    dll = (lib or load()).dll
    raw = np.frombuffer(version_index, np.uint8)
    n, target = C.c_uint32(0), C.c_uint32(0)
    err = dll.lthip_restore_asset_sizes(raw.ctypes.data if len(raw) else None, len(raw), None, C.byref(n), C.byref(target))
    if err:
        raise LongtailHipError(err, "lthip_restore_asset_sizes")
    sizes = np.zeros(n.value, np.uint64)
    err = dll.lthip_restore_asset_sizes(raw.ctypes.data, len(raw), sizes.ctypes.data if len(sizes) else None, C.byref(n), C.byref(target))
    if err:
        raise LongtailHipError(err, "lthip_restore_asset_sizes")
    return sizes, int(target.value)


def restore_rank_windows(job_asset, job_offset, job_size, job_rank, rank: int, align: int = 1, lib: Optional[HipLib] = None):
    """lthip_restore_rank_windows, host only: the jobs of `rank` (lthip_make_jobs / lthip_partition_jobs tables) as windows into a dense
    output of that rank's own -> ((n, 4) uint64 rows of (asset, offset, length, dst), out_bytes): what Restore(windows=...) takes."""
    dll = (lib or load()).dll
    ja, jo, js, jr = _u32arr(job_asset), _u64arr(job_offset), _u64arr(job_size), _u32arr(job_rank)
    assert len(ja) == len(jo) == len(js) == len(jr)
    ptrs = [x.ctypes.data if len(x) else None for x in (ja, jo, js, jr)]
    n, total = C.c_uint64(0), C.c_uint64(0)
    err = dll.lthip_restore_rank_windows(len(ja), *ptrs, rank, align, None, 0, C.byref(n), C.byref(total))
    if err:
        raise LongtailHipError(err, "lthip_restore_rank_windows")
    table = np.zeros(n.value, RESTORE_WINDOW_DTYPE)
    err = dll.lthip_restore_rank_windows(len(ja), *ptrs, rank, align, table.ctypes.data if len(table) else None, len(table), C.byref(n),
                                         C.byref(total))
    if err:
        raise LongtailHipError(err, "lthip_restore_rank_windows")
    rows = np.stack([table["asset"].astype(np.uint64), table["offset"], table["length"], table["dst"]], axis=1) if len(table) else np.zeros((0, 4), np.uint64)
    return rows, int(total.value)


def restore_layout_in_place(base_vi: bytes, base_offsets, base_bytes: int, target_vi: bytes, align: int = 1, lib: Optional[HipLib] = None):
    """lthip_restore_layout_in_place, host only: where the target's assets go in the buffer the base lies restored in -- unchanged assets
    keep their offsets, the others fill the gaps first fit or are appended -> (target offsets: uint64 array, total bytes, kept assets)."""
    dll = (lib or load()).dll
    a, b, offs = np.frombuffer(base_vi, np.uint8), np.frombuffer(target_vi, np.uint8), _u64arr(base_offsets)
    n = int(np.frombuffer(target_vi[12:16], np.uint32)[0]) if len(target_vi) >= 16 else 0
    out = np.zeros(max(n, 1), np.uint64)
    count, total, kept = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    err = dll.lthip_restore_layout_in_place(a.ctypes.data if len(a) else None, len(a), offs.ctypes.data, int(base_bytes),
                                            b.ctypes.data if len(b) else None, len(b), align, out.ctypes.data, C.byref(count), C.byref(total),
                                            C.byref(kept))
    if err:
        raise LongtailHipError(err, "lthip_restore_layout_in_place")
    return out[: count.value], int(total.value), int(kept.value)


class Plan:
    def __init__(self, ctx: Context, part_offsets, part_sizes, min_chunk: int, avg_chunk: int, max_chunk: int):
        self.ctx = ctx
        o, s = _u64arr(part_offsets), _u64arr(part_sizes)
        assert len(o) == len(s)
        self.nparts = len(o)
        h = C.c_void_p()
        err = ctx.lib.dll.lthip_plan_create(ctx.h, self.nparts, o.ctypes.data, s.ctypes.data, min_chunk, avg_chunk,
                                            max_chunk, C.byref(h))
        ctx._check(err, "lthip_plan_create")
        self.h = h
        self.capacity = int(ctx.lib.dll.lthip_plan_chunk_capacity(h))
        self.total_bytes = int(s.sum()) if len(s) else 0

    @property
    def slices(self) -> int:
        """How many slices chunk_hash runs this plan in on two streams (1 = the single pass, also what a walked plan runs as; 2 for tile-scan plans,
        LTHIP_SLICES in the ablation build): per-kernel timings of scan and leaf hashing of a sliced call overlap."""
        return int(self.ctx.lib.dll.lthip_plan_slices(self.h))

    @property
    def walked_scans(self) -> int:
        """How many of the plan's `slices` scans are walking scans (a wave per part, chunk by chunk); 0 = the tile scan."""
        return int(self.ctx.lib.dll.lthip_plan_walked_scans(self.h))

    def reaim(self, part_offsets, part_sizes):
        """The plan aimed at another set of parts (lthip_plan_reaim): no more parts / 16 KiB tiles than it was created with; the part
        tables are recomputed and rewritten on the context's stream, nothing is allocated or waited for."""
        o, s = _u64arr(part_offsets), _u64arr(part_sizes)
        assert len(o) == len(s)
        self.ctx._check(self.ctx.lib.dll.lthip_plan_reaim(self.ctx.h, self.h, len(o), o.ctypes.data, s.ctypes.data), "lthip_plan_reaim")
        self.nparts = len(o)
        self.capacity = int(self.ctx.lib.dll.lthip_plan_chunk_capacity(self.h))
        self.total_bytes = int(s.sum()) if len(s) else 0

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.dll.lthip_plan_destroy(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_blocks(lens: np.ndarray, max_block_size: int, max_chunks_per_block: int, lib: Optional[HipLib] = None) -> np.ndarray:
    """block start indices (+ end) for chunk lengths `lens` (uint32), Longtail_CreateStoreIndex's greedy rule."""
    lib = lib or load()
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    cap = len(lens) + 2
    starts = np.zeros(cap, dtype=np.uint64)
    nb = C.c_uint64(0)
    err = lib.dll.lthip_pack_blocks(len(lens), lens.ctypes.data, max_block_size, max_chunks_per_block, starts.ctypes.data, cap,
                                    C.byref(nb))
    if err:
        raise LongtailHipError(err, "lthip_pack_blocks")
    return starts[: nb.value + 1].astype(np.int64)


class BatchPacker:
    """Resumable greedy packing (lthip_pack_blocks_batch): next() -> (starts[n+1], sizes[n]) of the next batch of blocks, or
    None when every chunk is packed.  The work arrays are allocated once."""

    def __init__(self, lens: np.ndarray, max_block_size: int, max_chunks_per_block: int, max_batch_bytes: int, arena_bytes: int,
                 bound_div: int, bound_add: int, lib: Optional[HipLib] = None):
        self.lib = lib or load()
        self.lens = np.ascontiguousarray(lens, dtype=np.uint32)
        self.args = (max_block_size, max_chunks_per_block, max_batch_bytes, arena_bytes, bound_div, bound_add)
        self.pos = 0
        # a batch of B bytes holds at most B / (limit/2) + 2 blocks that were closed by size, or one per max_chunks chunks
        self.cap = int(min(len(self.lens), max_batch_bytes // max(1, max_block_size // 2) + len(self.lens) // max_chunks_per_block + 8) + 2)
        self.starts = np.empty(self.cap, dtype=np.uint64)
        self.sizes = np.empty(self.cap, dtype=np.uint64)

    def next(self):
        if self.pos >= len(self.lens):
            return None
        nb, nxt = C.c_uint64(0), C.c_uint64(0)
        mb, mc, bb, ab, bd, ba = self.args
        err = self.lib.dll.lthip_pack_blocks_batch(len(self.lens), self.lens.ctypes.data, self.pos, mb, mc, bb, ab, bd, ba,
                                                   self.starts.ctypes.data, self.sizes.ctypes.data, self.cap, C.byref(nb), C.byref(nxt))
        if err:
            raise LongtailHipError(err, "lthip_pack_blocks_batch")
        self.pos = nxt.value
        n = nb.value
        return self.starts[: n + 1].astype(np.int64), self.sizes[:n].astype(np.int64)


def chunker_params(target_chunk_size: int, chunker_min: int = 48):
    """min/avg/max as DynamicChunking derives them (src/longtail.c:1985-1987, 2111-2113)."""
    mn = max(chunker_min, target_chunk_size // 8)
    av = max(chunker_min, target_chunk_size // 2)
    mx = max(chunker_min, target_chunk_size * 2)
    return mn, av, mx
