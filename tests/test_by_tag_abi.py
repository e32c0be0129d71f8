"""CPU-only checks of the per-tag codec interface (include/longtail_hip.h, TAGS AND CODECS): the new entry points are declared and
exported by both builds, the gfx950 code object holds the raw-copy kernels, lthip_block_index_size is the BlockIndex's size, and
lthip_ingest_stream_arena_bound knows LTHIP_CODEC_NONE and LTHIP_CODEC_BY_TAG.  The ABI version stays 4: an enum value was added behind
the existing ones, no struct changed."""
import ctypes as C
import subprocess

import pytest

from longtail_amd.lib import CODECS, IngestConfig
from tests.test_abi import declared_symbols

NEW_SYMBOLS = ["lthip_block_index_size", "lthip_write_raw_block_images"]
RAW_KERNELS = ["k_raw_runs", "k_raw_copy"]
# (slice bytes, slice chunks) x (max_block_size, max_chunks_per_block)
SLICES = [(0, 0), (1, 1), (48, 1), (262144, 300), (8 << 20, 1024), (3 << 30, 2_000_000)]
BLOCKS = [(262144, 16), (1 << 20, 64), (8 << 20, 1024)]


def cfg_of(codec, max_block, max_chunks, tag=0):
    return IngestConfig(65536, 0x626C6B33, max_block, max_chunks, tag, CODECS[codec], 0)


def test_codec_names():
    assert CODECS == {"none": 0, "lz4": 1, "zstd": 2, "by-tag": 3}


def test_entry_points_are_declared_and_exported(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_code_object_holds_the_raw_copy_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in RAW_KERNELS:
        assert k in text, k


def test_block_index_size(hiplib):
    d = hiplib.dll
    for n in (0, 1, 2, 1024):
        assert d.lthip_block_index_size(n) == 20 + 12 * n == d.lthip_stored_block_header_size(n) - 8


def test_null_context_is_refused(hiplib):
    assert hiplib.dll.lthip_write_raw_block_images(None, 0, None, None, None, None, None, 0x626C6B33, None, None) != 0


@pytest.mark.parametrize("max_block,max_chunks", BLOCKS)
def test_arena_bound_of_raw_blocks_is_the_slot_arithmetic(hiplib, max_block, max_chunks):
    """LTHIP_CODEC_NONE: an image slot is round64(lthip_block_index_size(n) + raw).  A call closes blocks of at most
    R = slice_bytes + L bytes (L = max_block_size * 1.1, the block carried in) in N = slice_chunks + max_chunks_per_block chunks, at most N
    blocks; round64(x) <= x + 63 and lthip_block_index_size(n) = 20 + 12 n, so the slots sum to at most R + N * (20 + 12 + 63) =
    R + N * (lthip_block_index_size(1) + 63): one block's slot arithmetic, counted once per chunk.  The bound is exactly that -- and so it
    holds one block of n chunks and raw bytes, for every n and raw a block can have."""
    d = hiplib.dll
    limit = max_block + max_block // 10
    bis = d.lthip_block_index_size
    for slice_bytes, slice_chunks in SLICES:
        got = int(d.lthip_ingest_stream_arena_bound(C.byref(cfg_of("none", max_block, max_chunks)), slice_bytes, slice_chunks))
        assert got == slice_bytes + limit + (slice_chunks + max_chunks) * (int(bis(1)) + 63), (slice_bytes, slice_chunks)
    for n, raw in ((1, 1), (1, limit), (max_chunks, limit), (max_chunks, max_chunks)):
        slot = (int(bis(n)) + raw + 63) // 64 * 64
        assert slot <= int(d.lthip_ingest_stream_arena_bound(C.byref(cfg_of("none", max_block, max_chunks)), 0, 0)), (n, raw)


@pytest.mark.parametrize("max_block,max_chunks", BLOCKS)
def test_arena_bound_by_tag_is_no_less_than_any_one_codecs(hiplib, max_block, max_chunks):
    d = hiplib.dll
    for slice_bytes, slice_chunks in SLICES:
        one = {c: int(d.lthip_ingest_stream_arena_bound(C.byref(cfg_of(c, max_block, max_chunks)), slice_bytes, slice_chunks))
               for c in ("none", "lz4", "zstd")}
        by_tag = int(d.lthip_ingest_stream_arena_bound(C.byref(cfg_of("by-tag", max_block, max_chunks)), slice_bytes, slice_chunks))
        assert all(v > 0 for v in one.values()) and by_tag >= max(one.values()), (slice_bytes, slice_chunks, one, by_tag)
    # a slot of any of the three codecs fits the per-slot arithmetic the bound is made of: header + raw + raw / 255 + 64, rounded
    for raw in (0, 1, 255, 65536, 131071, 131072, max_block + max_block // 10):
        m = raw + raw // 255 + 64
        assert m >= int(d.lthip_lz4_bound(raw)) and m >= int(d.lthip_zstd_bound(raw)) and m >= raw
    # parameters no session would take
    assert d.lthip_ingest_stream_arena_bound(C.byref(IngestConfig(65536, 0, max_block, max_chunks, 0, 4, 0)), 0, 0) == 0
