"""CPU-only checks of the one-file archive's interface (include/longtail_hip.h, "one-file archives"): the entry points are declared and
exported by both builds, the ABI version stays 4, the package exports the new names, the code object holds the two new kernels; and the
index format (longtail_amd/csrc/archive_layout.h) against the reference (Longtail_CreateArchiveIndex / Longtail_ReadArchiveIndex through
ctypes on oracle/_ref, skipped where it is not built) and against a Python reading of the layout.  Every comparison is equality."""
import ctypes as C
import errno
import subprocess
from pathlib import Path

import numpy as np
import pytest

from longtail_amd.lib import Archive, LongtailHipError, Restore, archive_index_size, archive_peek, archive_write_index
from tests._libs import have_ref
from tests.archive_util import LZ4, RefArchive, header_bytes, parts_of_index
from tests.restore_util import BLK3, build_store_index, build_version_index
from tests.test_abi import declared_symbols

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["lthip_archive_index_size", "lthip_archive_write_index", "lthip_archive_peek", "lthip_archive_open", "lthip_archive_close",
               "lthip_archive_store_index", "lthip_archive_version_index", "lthip_archive_block_count", "lthip_archive_block_offsets",
               "lthip_archive_block_sizes", "lthip_archive_body_bytes", "lthip_archive_writer_create", "lthip_archive_writer_destroy",
               "lthip_archive_writer_append", "lthip_archive_writer_blocks", "lthip_archive_writer_finish", "lthip_restore_archive_blocks",
               "lthip_restore_archive_scratch_bound", "lthip_restore_archive_ranges"]
KERNELS = ["k_archive_pack", "k_restore_check_images_any"]
UNKNOWN = 0xFFFFFFFFFFFFFFFF


def indexes(nb, chunks_per_block, path_len, tags=None):
    """A StoreIndex of nb blocks of chunks_per_block chunks (block b tagged tags[b]) and a VersionIndex of one asset per block plus one
    whose path is path_len characters long."""
    m = nb * chunks_per_block
    hashes, sizes = np.arange(1000, 1000 + m, dtype=np.uint64), np.arange(1, m + 1, dtype=np.uint32) % 97 + 1
    tags = [0] * nb if tags is None else tags
    blocks = [(0xAA00 + b, tags[b], list(range(b * chunks_per_block, (b + 1) * chunks_per_block))) for b in range(nb)]
    names = [f"a{b}" for b in range(nb)] + ["p" * path_len]
    vi = build_version_index(BLK3, 32768, names, [cs for _, _, cs in blocks] + [[]], hashes, sizes)
    return build_store_index(BLK3, blocks, hashes, sizes), vi, [header_bytes(chunks_per_block, t) + 5 for t in tags]


def test_entry_points_are_declared_and_exported(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_the_code_object_holds_the_new_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    assert not [k for k in KERNELS if k not in text]
    assert "gfx950" in text


def test_the_package_exports_the_new_names_and_the_layout_is_host_code():
    import longtail_amd
    from longtail_amd import lib

    assert longtail_amd.Archive is lib.Archive and longtail_amd.ArchiveWriter is lib.ArchiveWriter
    for name in ("archive_blocks", "archive_scratch_bound", "archive_ranges"):
        assert callable(getattr(lib.Restore, name))
    for name in ("append", "blocks", "finish", "close"):
        assert callable(getattr(lib.ArchiveWriter, name))
    header = (ROOT / "include" / "longtail_hip.h").read_text()
    assert "one-file archives" in header
    layout = (ROOT / "longtail_amd" / "csrc" / "archive_layout.h").read_text().lower()
    for allowed in ("archive.hip", "restore.hip", "longtail_hip.h", "a line of hip", "lthip_archive"):
        layout = layout.replace(allowed, "")
    assert "hip" not in layout, "archive_layout.h is host code: a stand-alone program includes it alone"


def test_null_handles_are_refused_without_a_device(hiplib):
    dll = hiplib.dll
    n, h = C.c_uint64(0xEE), C.c_void_p(0x1234)
    assert dll.lthip_archive_index_size(None, 0, None, 0, C.byref(n)) == errno.EINVAL
    assert dll.lthip_archive_write_index(None, 0, None, 0, None, None, None, 0) == errno.EINVAL
    assert dll.lthip_archive_peek(None, C.byref(n)) == errno.EINVAL
    assert dll.lthip_archive_open(None, 0, 0, C.byref(h)) == errno.EINVAL and not h.value, "*out is cleared"
    assert dll.lthip_archive_close(None) is None
    assert dll.lthip_archive_block_count(None) == 0 and not dll.lthip_archive_block_offsets(None) and not dll.lthip_archive_store_index(None, None)
    h = C.c_void_p(0x1234)
    assert dll.lthip_archive_writer_create(None, C.byref(h)) == errno.EINVAL and not h.value
    assert dll.lthip_archive_writer_destroy(None) is None
    assert dll.lthip_archive_writer_append(None, None, 0, None, None, None, 0, C.byref(n)) == errno.EINVAL
    assert dll.lthip_archive_writer_blocks(None, None, None, None, None) == errno.EINVAL
    assert dll.lthip_archive_writer_finish(None, None, 0, None, 0, None, 0, C.byref(n)) == errno.EINVAL
    d, nx = C.c_uint32(0xEE), C.c_uint64(0xEE)
    assert dll.lthip_restore_archive_blocks(None, None, None, 0, 0, None, 0, None, C.byref(d), C.byref(nx)) == errno.EINVAL
    assert dll.lthip_restore_archive_scratch_bound(None, None, 0, 0) == 0
    assert dll.lthip_restore_archive_ranges(None, None, 0, None, 0, C.byref(n)) == errno.EINVAL
    assert n.value == 0xEE and d.value == 0xEE and nx.value == 0xEE, "a refused call writes nothing"


@pytest.mark.parametrize("nb,per_block", [(3, 2), (2, 2), (1, 1), (4, 3), (0, 0)])
def test_write_index_is_the_layout_and_open_reads_it_back(hiplib, nb, per_block):
    """nb + m odd and even (the u64 table 4- or 8-byte aligned), every pad length 0..7 by the last path's length, no blocks at all."""
    pads = set()
    for path_len in range(1, 9):
        si, vi, sizes = indexes(nb, per_block, path_len, tags=[LZ4 if b % 2 else 0 for b in range(nb)])
        offsets = np.array([7 + 1000 * ((b * 5) % max(nb, 1)) for b in range(nb)], np.uint64)  # shuffled, odd
        bare = 8 + len(si) + 12 * nb + len(vi)
        assert archive_index_size(si, vi) == (bare + 7) // 8 * 8
        index = archive_write_index(si, vi, offsets, sizes)
        p = parts_of_index(index)
        assert (p["version"], p["stored"], p["si"]) == (1, len(index), si) and p["tables_at"] % 8 == (0 if (nb + nb * per_block) % 2 == 0 else 4)
        assert (p["offsets"] == offsets).all() and (p["sizes"] == sizes).all()
        assert p["vi"][: len(vi)] == vi and p["vi"][len(vi) :] == bytes(len(index) - bare), "our pad is zero"
        pads.add(len(index) - bare)
        assert archive_peek(index[:8]) == len(index)
        for body in (None, int(max([int(o) + z for o, z in zip(offsets, sizes)], default=0))):
            a = Archive(index, body)
            assert a.store_index == si and a.version_index == p["vi"] and a.block_count == nb
            assert (a.block_offsets == offsets).all() and (a.block_sizes == sizes).all()
            assert a.body_bytes == max([int(o) + z for o, z in zip(offsets, sizes)], default=0)
            (offs, total), (want_offs, want_total) = Restore.layout(a.version_index), Restore.layout(vi)
            assert (offs == want_offs).all() and total == want_total, "the VersionIndex with its pad is the VersionIndex"
            a.close()
    assert pads == set(range(8))


def corrupt(index, at, value, width=4):
    b = bytearray(index)
    b[at : at + width] = int(value).to_bytes(width, "little")
    return bytes(b)


def open_code(index, body=None):
    try:
        Archive(index, body).close()
        return 0
    except LongtailHipError as e:
        return e.code


def test_open_refuses_every_prefix_and_every_listed_corruption(hiplib):
    si, vi, sizes = indexes(3, 2, 5, tags=[0, LZ4, 0])
    offsets = np.array([100, 0, 50], np.uint64)
    index = archive_write_index(si, vi, offsets, sizes)
    p = parts_of_index(index)
    body = 100 + sizes[0]
    assert open_code(index, body) == 0 and open_code(index) == 0
    for k in range(len(index)):
        assert open_code(index[:k], body) == errno.EBADF, k
    t = p["tables_at"]
    cases = {
        "over-long": index + bytes(8),
        "another version": corrupt(index, 0, 2),
        "stored size": corrupt(index, 4, len(index) - 8),
        "block count leaves the index": corrupt(index, 16, 0x7FFFFFFF),
        "chunk count leaves the index": corrupt(index, 20, 0x7FFFFFFF),
        "store index version": corrupt(index, 8, 5),
        "store index: a block's chunks leave the chunk list": corrupt(index, 8 + 16 + 3 * 8 + 6 * 8 + 3 * 4, 9),
        "block below its header (raw)": corrupt(index, t + 24, header_bytes(2, 0) - 1),
        "block below its header (tagged)": corrupt(index, t + 28, header_bytes(2, LZ4) - 1),
        "offset + size wraps": corrupt(index, t, 2**64 - 4, 8),
        "version index version": corrupt(index, p["vi_at"], 7),
        "version index: asset count leaves the index": corrupt(index, p["vi_at"] + 12, 0x7FFFFFFF),
        "version index: the last path loses its terminator": index[: p["vi_at"] + len(vi) - 1] + b"x" * (len(index) - p["vi_at"] - len(vi) + 1),
    }
    for what, bad in cases.items():
        assert open_code(bad, None if what == "offset + size wraps" else body) == errno.EBADF, what
    assert open_code(index, body - 1) == errno.EBADF, "a block whose offset + size leaves body_bytes"
    assert open_code(corrupt(index, t + 8, body, 8), body) == errno.EBADF, "an offset at the body's end"
    for first8 in (index[:8], corrupt(index, 0, 2)[:8]):
        if first8 == index[:8]:
            assert archive_peek(first8) == len(index)
        else:
            with pytest.raises(LongtailHipError) as e:
                archive_peek(first8)
            assert e.value.code == errno.EBADF


def test_sizes_that_do_not_fit_are_refused_not_truncated(hiplib):
    si, vi, sizes = indexes(2, 2, 3)
    n = C.c_uint64(0xEE)
    bsi, bvi = np.frombuffer(si, np.uint8), np.frombuffer(vi, np.uint8)
    # a claimed VersionIndex of 4 GiB cannot be offered; a short capacity can: ENOMEM, nothing written
    out = np.full(archive_index_size(si, vi), 0xEE, np.uint8)
    o, z = np.zeros(2, np.uint64), np.array(sizes, np.uint32)
    assert hiplib.dll.lthip_archive_write_index(bsi.ctypes.data, len(bsi), bvi.ctypes.data, len(bvi), o.ctypes.data, z.ctypes.data, out.ctypes.data,
                                                len(out) - 1) == errno.ENOMEM
    assert (out == 0xEE).all()
    assert hiplib.dll.lthip_archive_index_size(bsi.ctypes.data, len(bsi) - 1, bvi.ctypes.data, len(bvi), C.byref(n)) == errno.EBADF
    assert hiplib.dll.lthip_archive_index_size(bsi.ctypes.data, len(bsi), bvi.ctypes.data, len(bvi) - 1, C.byref(n)) == errno.EBADF
    assert n.value == 0xEE


# ---- against the reference ----

needs_ref = pytest.mark.skipif(not have_ref(), reason="oracle/_ref/liblongtail_ref.so not built (needs /root/reference at build time)")


@needs_ref
@pytest.mark.parametrize("nb,per_block", [(3, 2), (2, 2), (1, 1), (4, 3)])
def test_write_index_equals_create_archive_index_up_to_the_pad(hiplib, ref, nb, per_block):
    ra = RefArchive(ref)
    pads = set()
    for path_len in range(1, 9):
        si, vi, sizes = indexes(nb, per_block, path_len, tags=[LZ4 if b % 2 else 0 for b in range(nb)])
        offsets = np.array([3 + 999 * ((b * 3) % nb) for b in range(nb)], np.uint64)
        theirs = ra.create(si, vi, offsets, sizes)
        assert isinstance(theirs, bytes), theirs
        ours = archive_write_index(si, vi, offsets, sizes)
        bare = 8 + len(si) + 12 * nb + len(vi)
        assert len(ours) == len(theirs) and ours[:bare] == theirs[:bare] and ours[bare:] == bytes(len(ours) - bare)
        pads.add(len(ours) - bare)
    assert pads == set(range(8))


@needs_ref
def test_the_reference_on_an_empty_store_index(hiplib, ref):
    """A StoreIndex without blocks: the reference accepts it (Longtail_CreateArchiveIndex returns 0), and the bytes are equal."""
    si, vi, _ = indexes(0, 0, 4)
    theirs = RefArchive(ref).create(si, vi, [], [])
    assert isinstance(theirs, bytes), f"the reference refuses an empty StoreIndex with {theirs}"
    ours = archive_write_index(si, vi, [], [])
    bare = 8 + len(si) + len(vi)
    assert len(ours) == len(theirs) and ours[:bare] == theirs[:bare]


@needs_ref
def test_read_archive_index_reads_ours_and_open_reads_theirs(hiplib, ref, tmp_path):
    ra = RefArchive(ref)
    si, vi, sizes = indexes(5, 3, 6, tags=[0, LZ4, 0, LZ4, 0])
    offsets = np.array([4001, 13, 999, 2002, 3003], np.uint64)  # shuffled, odd
    ours = archive_write_index(si, vi, offsets, sizes)
    body = np.arange(4001 + sizes[0], dtype=np.uint32).astype(np.uint8).tobytes()
    path = tmp_path / "ours.la"
    path.write_bytes(ours + body)
    got = ra.read(str(path))
    assert isinstance(got, dict), got
    p = parts_of_index(ours)
    assert got["index"] == ours and (got["offsets"] == offsets).all() and (got["sizes"] == sizes).all() and got["vi_at"] == p["vi_at"]
    assert got["index"][8 : 8 + len(si)] == si and got["index"][got["vi_at"] :][: len(vi)] == vi
    theirs = ra.create(si, vi, offsets, sizes)
    a = Archive(theirs, len(body))
    assert a.store_index == si and a.version_index[: len(vi)] == vi and len(a.version_index) - len(vi) == len(theirs) - p["vi_at"] - len(vi)
    assert (a.block_offsets == offsets).all() and (a.block_sizes == sizes).all() and a.body_bytes == len(body)
    assert (Restore.layout(a.version_index)[0] == Restore.layout(vi)[0]).all(), "the pad behind the name data is accepted, whatever it holds"
    a.close()
