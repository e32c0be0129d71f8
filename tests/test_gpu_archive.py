"""-m gpu: one-file archives (lthip_archive_*, lthip_restore_archive_*, include/longtail_hip.h "one-file archives").

  * pack: k_archive_pack lays images densely, destination offsets at every residue mod 16, over three append calls and an empty one; the
    last image ends at the last byte of the destination, a sentinel behind bytes_written stays, the recorded offsets continue across calls
  * the check at any byte position: a hand-built store (tests/archive_util.py) with blocks of 1, 64, 65 and 130 chunks, raw and tagged,
    delivered at every residue 0..7 with the last image ending at the window's last byte; every header field corrupted in turn at an odd
    residue; an image shorter than its header
  * round trips: a tree of small 'mixed' files through the stream session in three slices, for NONE, LZ4, zstd and BY_TAG -> writer ->
    archive -> (with the reference) Longtail_ReadArchiveIndex and refh_open_stored_block on every block -> restore with the body in one
    window and in windows cut mid-block that follow next_byte, verify off and on
  * an archive the reference's index writer and codecs wrote (tests/golden/archive_ref.npz, tools/gen_archive_golden.py): blocks in
    shuffled order at odd offsets
  * with a block cache a second session is served without a window; a window session reads only lthip_restore_archive_ranges; with a
    base only the blocks it does not feed are taken from the archive
  * refusals: scratch below the bound, a window without a complete block, a bad block before good ones, the writer's

In every restore the output buffer is filled with 0xA5 first and compared WHOLE with what is expected.  Every comparison is equality."""
import ctypes as C
import errno

import numpy as np
import pytest
import torch

from longtail_amd.dist import JobPartition
from longtail_amd.lib import (RESTORE_BAD_HEADER, Archive, ArchiveWriter, BlockCache, LongtailHipError, Restore, archive_peek,
                              archive_write_index)
from tests._libs import GOLDEN, have_ref
from tests.archive_util import (LZ4, RefArchive, expected_output, hand_store, header_bytes, offsets_at_residue, parts_of_index, place)
from tests.restore_util import BLK3, build_store_index, build_version_index, parse_store_index
from tests.test_gpu_ingest_stream import _sessions, chunk_jobs, index_buffers, open_stream, slices_of, stream_tree
from tests.test_gpu_raw_blocks import ref_opens_raw_image

pytestmark = pytest.mark.gpu

FILL = 0xA5
ZTD2, ZTD4 = 0x7A746432, 0x7A746434
_open, _packed = [], {}


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    yield
    while _open:
        _open.pop().close()
    while _sessions:
        _sessions.pop().close()


def keep(obj):
    _open.append(obj)
    return obj


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def round64(n):
    return (n + 63) // 64 * 64


@pytest.fixture(scope="module")
def store(oracle):
    return hand_store(oracle)


def archive_of(st, offsets, images=None, body_bytes=None):
    images = st["images"] if images is None else images
    body = place(images, offsets, body_bytes)
    index = archive_write_index(st["si"], st["vi"], offsets, [len(i) for i in images])
    return keep(Archive(index, len(body))), body


def session(gpu, a, verify=True, align=1):
    offs, total = Restore.layout(a.version_index, align)
    rs = keep(Restore(gpu, a.version_index, a.store_index, offs, total, verify=verify))
    return rs, offs, total, torch.full((max(total, 1),), FILL, dtype=torch.uint8, device="cuda")


def feed(rs, a, body, first, n, out, scratch_delta=0):
    """One lthip_restore_archive_blocks call with body bytes [first, first + n) in a tensor of exactly n bytes and a scratch of exactly
    the bound."""
    window = dev(body[first : first + n]) if n else None
    bound = rs.archive_scratch_bound(a, first, n) + scratch_delta
    scratch = torch.full((bound,), 0x3C, dtype=torch.uint8, device="cuda") if bound > 0 else None
    return rs.archive_blocks(a, window, first, scratch, out, window_bytes=n)


# ---- 1. pack ----


def test_pack_lays_the_images_densely_at_every_residue(gpu):
    rng = np.random.default_rng(1)
    sizes = [17, 4097, 33, 300001, 1, 65, 129, 49, 1041, 81, 97, 113, 262145, 145, 161, 177, 193, 209, 524289, 225]  # all 1 mod 16
    images = [rng.integers(0, 256, n).astype(np.uint8) for n in sizes]
    calls = [list(range(0, 16)), [], [16, 17, 18], [19]]
    assert {sum(sizes[:k]) % 16 for k in range(16)} == set(range(16)), "the first call's destination offsets take every residue"
    w = keep(ArchiveWriter(gpu))
    body, cursor = [], 0
    for k, call in enumerate(calls):
        # the arena as an ingest session leaves it: 8-byte aligned images with room between them, the last one at the arena's end
        src_offs, at = [], 8
        for b in call:
            src_offs.append(at)
            at = (at + sizes[b] + 7) // 8 * 8 + 8 * (b % 3)
        arena_bytes = src_offs[-1] + sizes[call[-1]] if call else 8
        arena = np.full(arena_bytes, 0x77, np.uint8)
        for o, b in zip(src_offs, call):
            arena[o : o + sizes[b]] = images[b]
        total = sum(sizes[b] for b in call)
        exact = k % 2 == 0  # the last image ends at the last byte of d_dst / a sentinel lies behind bytes_written
        dst = torch.full((total + (0 if exact else 64),), 0xC3, dtype=torch.uint8, device="cuda") if total or not exact else None
        if total:
            with pytest.raises(LongtailHipError) as e:
                w.append(dev(arena), src_offs, [sizes[b] for b in call], dst, dst_capacity=total - 1)
            assert e.value.code == errno.ENOMEM and w.blocks()[2] == cursor, "refused before any work: the cursor stays"
        n = w.append(dev(arena), src_offs, [sizes[b] for b in call], dst, dst_capacity=total)
        gpu.sync()
        assert n == total
        host = dst.cpu().numpy() if dst is not None else np.zeros(0, np.uint8)
        assert (host[n:] == 0xC3).all(), "nothing is written at or beyond d_dst + bytes_written"
        body.append(host[:n].copy())
        cursor += total
    offs, got_sizes, body_bytes = w.blocks()
    assert (offs == np.concatenate([[0], np.cumsum(sizes)[:-1]])).all() and (got_sizes == sizes).all() and body_bytes == sum(sizes) == cursor
    assert (np.concatenate(body) == np.concatenate(images)).all()


# ---- 2. the check at any byte position ----


@pytest.mark.parametrize("residue", range(8))
def test_every_block_is_checked_and_restored_at_every_residue(gpu, store, residue):
    """The blocks in reverse order, every image at `residue` mod 8; the body ends with the last image: at the window's last byte."""
    images = store["images"]
    offsets = offsets_at_residue(images, residue, order=list(reversed(range(len(images)))), gap=3)
    a, body = archive_of(store, offsets)
    assert all(int(o) % 8 == residue for o in offsets) and len(body) == int(offsets[0]) + len(images[0])
    rs, offs, total, out = session(gpu, a)
    assert rs.archive_scratch_bound(a, 0, len(body)) == sum(round64(sum(store["lens"][c] for c in cs)) for _, t, cs in store["blocks"] if t)
    assert feed(rs, a, body, 0, len(body), out) == (len(images), len(body))
    code, res = rs.finish()
    assert (code, res.blocks_bad, res.blocks_delivered, res.chunks_mismatched) == (0, 0, len(images), 0)
    assert (rs.block_status(store["block_hashes"]) == 0).all()
    assert (out.cpu().numpy()[:total] == expected_output(store, offs, total)).all()


def field_offset(field, n):
    """Where a header field lies in a stored-block image of n chunks."""
    return {"block hash, low": 0, "block hash, high": 7, "hash identifier": 8, "chunk count": 12, "tag": 16, "first chunk hash": 20,
            "last chunk hash, high": 20 + 8 * (n - 1) + 7, "size of chunk 63 or the last": 20 + 8 * n + 4 * min(63, n - 1),
            "last chunk size": 20 + 8 * n + 4 * (n - 1) + 3, "raw size": 20 + 12 * n + 1, "compressed size": 24 + 12 * n}[field]


FIELDS = ["block hash, low", "block hash, high", "hash identifier", "chunk count", "tag", "first chunk hash", "last chunk hash, high",
          "size of chunk 63 or the last", "last chunk size", "raw size", "compressed size"]


@pytest.mark.parametrize("field", FIELDS)
def test_a_corrupted_header_field_at_an_odd_residue_flags_the_block(gpu, store, field):
    """One bit of the field flipped in every block that has it (the [raw][compressed] words: the tagged ones), every image at residue 5."""
    tagged_only = field in ("raw size", "compressed size")
    images, bad = [], set()
    for b, image in enumerate(store["images"]):
        image = image.copy()
        if store["tags"][b] or not tagged_only:
            image[field_offset(field, store["counts"][b])] ^= 0x10
            bad.add(b)
        images.append(image)
    offsets = offsets_at_residue(images, 5, gap=1)
    a, body = archive_of(store, offsets, images)
    rs, offs, total, out = session(gpu, a)
    assert feed(rs, a, body, 0, len(body), out) == (len(images), len(body))
    code, res = rs.finish()
    good = set(range(len(images))) - bad
    assert (code, res.blocks_bad) == (errno.EBADF, len(bad))
    status = rs.block_status(store["block_hashes"])
    assert [int(s) for s in status] == [RESTORE_BAD_HEADER if b in bad else 0 for b in range(len(images))]
    assert (out.cpu().numpy()[:total] == expected_output(store, offs, total, good)).all(), "no byte of a bad block reaches d_out"


def test_an_image_shorter_than_its_header_is_bad_and_not_read(gpu, store):
    """The archive's own StoreIndex lists block 2 (64 chunks) with one chunk, so that its 40-byte image passes lthip_archive_open; the
    session was made from the true StoreIndex: 40 bytes are below that block's header.  The image lies at the window's last bytes."""
    blocks = [(h, t, cs[:1] if b == 2 else cs) for b, (h, t, cs) in enumerate(store["blocks"])]
    si_short = build_store_index(BLK3, blocks, store["hashes"], store["lens"])
    images = [i[:40] if b == 2 else i for b, i in enumerate(store["images"])]
    order = [b for b in range(len(images)) if b != 2] + [2]
    offsets = offsets_at_residue(images, 3, order=order)
    body = place(images, offsets)
    a = keep(Archive(archive_write_index(si_short, store["vi"], offsets, [len(i) for i in images]), len(body)))
    assert len(body) == int(offsets[2]) + 40 and header_bytes(64, 0) > 40 >= header_bytes(1, 0)
    offs, total = Restore.layout(store["vi"])
    rs = keep(Restore(gpu, store["vi"], store["si"], offs, total, verify=True))
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    assert feed(rs, a, body, 0, len(body), out) == (len(images), len(body))
    code, res = rs.finish()
    assert (code, res.blocks_bad) == (errno.EBADF, 1)
    assert [int(s) for s in rs.block_status(store["block_hashes"])] == [RESTORE_BAD_HEADER if b == 2 else 0 for b in range(len(images))]
    assert (out.cpu().numpy()[:total] == expected_output(store, offs, total, set(range(len(images))) - {2})).all()


# ---- 3. round trips of what the stream session wrote ----


def small_tree(oracle, target):
    """Thirty 'mixed' files of 1 byte .. 120 KB in four directories, an empty file among them."""
    rng = np.random.default_rng(3)
    files = [(f"d{i % 4}/f{i:02d}.bin", np.zeros(0, np.uint8) if i == 7 else oracle.synth(int(rng.integers(1, 120_000)), 300 + i, 1))
             for i in range(30)]
    paths = [n for n, _ in files]
    path_data = b"".join(p.encode() + b"\0" for p in paths)
    offs = np.array([sum(len(p) + 1 for p in paths[:a]) for a in range(len(paths))], np.uint32)
    sizes = np.array([len(d) for _, d in files], np.uint64)
    return dict(files=files, by_name=dict(files), paths=paths, sizes=sizes, offs=offs, perms=np.full(len(paths), 0o644, np.uint16),
                path_data=path_data, part=JobPartition(sizes, target, 1, "range"))


def packed(gpu, oracle, codec):
    """The tree through the stream session in three slices, every call's images appended by an ArchiveWriter as lthip_ingest_stream_images
    hands them out -> dict(tree, index, body, vi, si, offsets, sizes), once per codec."""
    if codec not in _packed:
        target, max_block, max_chunks = 4096, 65536, 32
        tree = small_tree(oracle, target)
        tags = None
        if codec == "by-tag":
            tags = np.array([(0, LZ4, ZTD2, ZTD4)[int(p[1])] for p in tree["paths"]], np.uint32)
        tag = {"none": None, "lz4": LZ4, "zstd": ZTD2, "by-tag": None}[codec]
        st = open_stream(gpu, stream_tree(tree, tags), target, max_block, max_chunks, codec, compression_type=tag)
        w = keep(ArchiveWriter(gpu))
        body, chunks_all = [], 0

        def drain(arena):
            _, offs, sizes = st.images()
            total = int(sizes.astype(np.int64).sum())
            dst = torch.full((total + 64,), 0xC3, dtype=torch.uint8, device="cuda")
            n = w.append(arena, offs, sizes, dst, dst_capacity=total)
            gpu.sync()
            host = dst.cpu().numpy()
            assert n == total and (host[n:] == 0xC3).all()
            body.append(host[:n].copy())

        for first_job, count in slices_of("three", tree["part"].job_count):
            sl = chunk_jobs(gpu, tree, target, first_job, count)
            arena = torch.zeros(max(64, st.arena_bound(sl["bytes"], sl["total"])), dtype=torch.uint8, device="cuda")
            st.slice(first_job, count, sl["dev"], sl["d_off"], sl["d_len"], sl["d_hash"], sl["d_first"], sl["total"], arena)
            drain(arena)
            chunks_all += sl["total"]
        arena = torch.zeros(st.arena_bound(0, 0), dtype=torch.uint8, device="cuda")
        vi, si = index_buffers(gpu, tree, chunks_all)
        res = st.finish(arena, vi, si)
        drain(arena)
        vi, si = bytes(vi.numpy()[: res.version_index_size]), bytes(si.numpy()[: res.store_index_size])
        offsets, sizes, body_bytes = w.blocks()
        assert len(offsets) == res.blocks > 8 and body_bytes == sum(len(b) for b in body)
        _packed[codec] = dict(tree=tree, index=w.finish(si, vi), body=np.concatenate(body), vi=vi, si=si, offsets=offsets, sizes=sizes)
    return _packed[codec]


def tree_output(tree, offs, total):
    out = np.full(total, FILL, np.uint8)
    for (_, data), off in zip(tree["files"], offs):
        out[int(off) : int(off) + len(data)] = data
    return out


@pytest.mark.parametrize("codec", ["none", "lz4", "zstd", "by-tag"])
def test_the_writers_archive_is_the_layout_and_the_reference_reads_it(gpu, oracle, codec, tmp_path):
    p = packed(gpu, oracle, codec)
    parts = parts_of_index(p["index"])
    assert (parts["version"], parts["stored"], parts["si"]) == (1, len(p["index"]), p["si"]) and parts["vi"][: len(p["vi"])] == p["vi"]
    assert (parts["offsets"] == p["offsets"]).all() and (parts["sizes"] == p["sizes"]).all() and not any(parts["vi"][len(p["vi"]) :])
    assert len({int(o) % 8 for o in p["offsets"]}) > 1, "about this test's input: the images do not all lie 8-byte aligned"
    if not have_ref():
        return
    from tests._libs import ref as _ref

    ref = _ref()
    path = tmp_path / "tree.la"
    path.write_bytes(p["index"] + p["body"].tobytes())
    got = RefArchive(ref).read(str(path))
    assert isinstance(got, dict), f"Longtail_ReadArchiveIndex: errno {got}"
    assert got["index"] == p["index"] and (got["offsets"] == p["offsets"]).all() and (got["sizes"] == p["sizes"]).all()
    si = parse_store_index(p["si"])
    for b, (o, z) in enumerate(zip(p["offsets"], p["sizes"])):
        image = p["body"][int(o) : int(o) + int(z)].copy()
        c0, n = int(si["block_offsets"][b]), int(si["block_counts"][b])
        h, s = np.ascontiguousarray(si["chunk_hashes"][c0 : c0 + n]), np.ascontiguousarray(si["chunk_sizes"][c0 : c0 + n])
        raw = int(s.astype(np.int64).sum())
        if int(si["block_tags"][b]) == 0:  # (a raw image has no [raw][compressed] words: Longtail_ReadStoredBlockFromBuffer alone)
            assert ref_opens_raw_image(ref, image) == raw, b
            continue
        out, n_out = np.zeros(raw + 8, np.uint8), C.c_uint64(0)
        err = ref.dll.refh_open_stored_block(image.ctypes.data, len(image), n, h.ctypes.data, s.ctypes.data, int(si["block_tags"][b]),
                                             out.ctypes.data, raw, C.byref(n_out))
        assert (err, n_out.value) == (0, raw), b


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("codec", ["none", "lz4", "zstd", "by-tag"])
def test_round_trip_in_one_window_and_in_windows_cut_mid_block(gpu, oracle, codec, verify):
    p = packed(gpu, oracle, codec)
    body = p["body"]
    assert archive_peek(p["index"][:8]) == len(p["index"])
    a = keep(Archive(p["index"], len(body)))
    # the body in one window
    rs, offs, total, out = session(gpu, a, verify, align=1)
    assert feed(rs, a, body, 0, len(body), out) == (len(p["offsets"]), len(body))
    code, res = rs.finish()
    assert (code, res.blocks_bad, res.bytes_written) == (0, 0, int(p["tree"]["sizes"].sum()))
    want = tree_output(p["tree"], offs, total)
    assert (out.cpu().numpy()[:total] == want).all()
    # windows of a sixth of the body (and no less than the largest image) that start where next_byte says: each holds at least the
    # block it starts with, and cuts the last one
    window = max(int(p["sizes"].max()), len(body) // 6) + 1
    assert window < len(body)
    rs, offs, total, out = session(gpu, a, verify, align=1)
    first, calls, delivered_all, cut = 0, 0, 0, 0
    while first < len(body):
        n = min(window, len(body) - first)
        delivered, nxt = feed(rs, a, body, first, n, out)
        assert delivered > 0 and first < nxt <= len(body)
        cut += nxt < first + n
        first, calls, delivered_all = nxt, calls + 1, delivered_all + delivered
        assert calls <= len(p["offsets"])
    assert delivered_all == len(p["offsets"]) and calls > 2 and cut > 0
    code, res = rs.finish()
    assert (code, res.blocks_bad) == (0, 0)
    assert (out.cpu().numpy()[:total] == want).all()


# ---- 4. an archive the reference wrote ----


def test_a_reference_written_archive_restores_to_its_assets(gpu):
    g = np.load(GOLDEN / "archive_ref.npz")
    archive, assets, sizes = g["archive"], g["assets"], g["asset_sizes"]
    index_bytes = archive_peek(archive[:8].tobytes())
    assert index_bytes == int(g["index_bytes"][0])
    body = archive[index_bytes:]
    a = keep(Archive(archive[:index_bytes].tobytes(), len(body)))
    order = np.argsort(a.block_offsets)
    assert all(int(o) % 2 for o in a.block_offsets) and (order != np.arange(len(order))).any(), "odd offsets, shuffled order"
    tags = parse_store_index(a.store_index)["block_tags"]
    assert sorted(set(int(t) for t in tags)) == [0, LZ4, ZTD2]
    for verify in (False, True):
        rs, offs, total, out = session(gpu, a, verify, align=16)
        assert feed(rs, a, body, 0, len(body), out) == (len(tags), len(body))
        code, res = rs.finish()
        assert (code, res.blocks_bad) == (0, 0)
        want, at = np.full(total, FILL, np.uint8), 0
        for off, n in zip(offs, sizes):
            want[int(off) : int(off) + int(n)] = assets[at : at + int(n)]
            at += int(n)
        assert (out.cpu().numpy()[:total] == want).all()


# ---- 5. with a cache, and a window session over the ranges ----


def test_a_second_session_is_served_from_the_cache_without_a_window(gpu, store):
    offsets = offsets_at_residue(store["images"], 1, gap=5)
    a, body = archive_of(store, offsets)
    cache = BlockCache(gpu, 16, 8192)
    try:
        rs, offs, total, out = session(gpu, a)
        rs.set_cache(cache)
        assert feed(rs, a, body, 0, len(body), out) == (8, len(body))
        assert rs.finish()[0] == 0 and rs.cache_stats()[2] == 8
        want = expected_output(store, offs, total)
        assert (out.cpu().numpy()[:total] == want).all()
        rs2, offs, total, out2 = session(gpu, a)
        rs2.set_cache(cache)
        assert len(rs2.needed_blocks()) == 0 and len(rs2.archive_ranges(a, 0)) == 0
        assert feed(rs2, a, body, 0, 0, out2) == (0, len(body)), "nothing is outstanding: no window is needed"
        rs2.from_cache(out2)
        assert rs2.finish()[0] == 0 and rs2.cache_stats()[0] == 8
        assert (out2.cpu().numpy()[:total] == want).all()
    finally:
        while _open:
            _open.pop().close()
        cache.close()


def test_a_window_session_reads_only_the_ranges(gpu, store):
    """Bytes [3, 23) of asset 2 and [0, 10) of asset 5: blocks 2 and 5 of eight.  The ranges at max_gap 0 are those two images; a reader
    that reads them and nothing else finishes the session."""
    offsets = offsets_at_residue(store["images"], 7, order=[5, 0, 1, 3, 4, 2, 6, 7], gap=9)
    a, body = archive_of(store, offsets)
    rs = keep(Restore(gpu, a.version_index, a.store_index, None, 64, verify=True, windows=[(2, 3, 20, 0), (5, 0, 10, 32)]))
    out = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
    ranges = rs.archive_ranges(a, 0)
    assert [tuple(int(x) for x in r) for r in ranges] == [(int(offsets[5]), len(store["images"][5])), (int(offsets[2]), len(store["images"][2]))]
    one = rs.archive_ranges(a, len(body))
    assert [tuple(int(x) for x in r) for r in one] == [(int(offsets[5]), int(offsets[2]) + len(store["images"][2]) - int(offsets[5]))]
    poisoned = np.full(len(body), 0x11, np.uint8)  # everything outside the ranges is not the archive's
    for first, n in ranges:
        poisoned[int(first) : int(first + n)] = body[int(first) : int(first + n)]
    got = [feed(rs, a, poisoned, int(first), int(n), out) for first, n in ranges]
    assert got == [(1, int(offsets[2])), (1, len(body))]
    assert len(rs.archive_ranges(a, 0)) == 0
    code, res = rs.finish()
    assert (code, res.blocks_bad, res.blocks_delivered) == (0, 0, 2)
    want = np.full(64, FILL, np.uint8)
    want[0:20], want[32:42] = store["files"][2][3:23], store["files"][5][0:10]
    assert (out.cpu().numpy() == want).all()


def test_with_a_base_only_the_blocks_it_does_not_feed_are_taken_from_the_archive(gpu, store):
    """The assets of blocks 0..3 lie restored in HBM as the base: their chunks are carried, and of the archive's eight blocks the session
    takes the other four, wherever they lie."""
    nbase = sum(store["counts"][:4])
    base_vi = build_version_index(BLK3, 32768, store["names"][:4], store["asset_chunks"][:4], store["hashes"][:nbase], store["lens"][:nbase])
    base_offsets, base_bytes = Restore.layout(base_vi, 16)
    base = np.full(base_bytes, 0x99, np.uint8)
    for off, data in zip(base_offsets, store["files"][:4]):
        base[int(off) : int(off) + len(data)] = data
    offsets = offsets_at_residue(store["images"], 6, order=[7, 2, 5, 0, 4, 1, 6, 3], gap=1)
    a, body = archive_of(store, offsets)
    offs, total = Restore.layout(a.version_index, 1)
    rs = keep(Restore(gpu, a.version_index, a.store_index, offs, total, verify=True, base=(base_vi, base_offsets, base_bytes)))
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    assert sorted(int(h) for h in rs.needed_blocks()) == sorted(int(h) for h in store["block_hashes"][4:])
    rs.carry(dev(base), out)
    assert feed(rs, a, body, 0, len(body), out) == (4, len(body))
    code, res = rs.finish()
    assert (code, res.blocks_bad, res.blocks_delivered, res.blocks_needed) == (0, 0, 4, 4) and res.base_occurrences > 0
    assert (out.cpu().numpy()[:total] == expected_output(store, offs, total)).all()


# ---- 6. refusals ----


def test_refusals_leave_the_session_usable_and_a_bad_block_does_not_stop_the_rest(gpu, store):
    images = [i.copy() for i in store["images"]]
    images[0][9] ^= 1  # block 0: its hash identifier
    offsets = offsets_at_residue(images, 3, gap=2)
    a, body = archive_of(store, offsets, images)
    rs, offs, total, out = session(gpu, a)
    # a window with no complete block
    assert feed(rs, a, body, 0, len(images[0]) + 2, out) == (0, int(offsets[0])), "block 0 lies at byte 3: its last byte is cut off"
    assert feed(rs, a, body, int(offsets[1]) + 1, len(body) - int(offsets[1]) - 1 - 1, out) == (5, int(offsets[0])), \
        "blocks 2..6: block 1 and block 7 are cut"
    # scratch below the bound: ENOMEM, nothing delivered, the session usable
    with pytest.raises(LongtailHipError) as e:
        feed(rs, a, body, 0, len(body), out, scratch_delta=-1)
    assert e.value.code == errno.ENOMEM
    assert [tuple(int(x) for x in r) for r in rs.archive_ranges(a, 0)] == [(int(offsets[b]), len(images[b])) for b in (0, 1, 7)]
    # the bad block first, the rest after it
    assert feed(rs, a, body, 0, int(offsets[1]), out) == (1, int(offsets[1]))
    assert feed(rs, a, body, int(offsets[1]), len(body) - int(offsets[1]), out) == (2, len(body))
    code, res = rs.finish()
    assert (code, res.blocks_bad, res.blocks_delivered) == (errno.EBADF, 1, 8)
    assert [int(s) for s in rs.block_status(store["block_hashes"])] == [RESTORE_BAD_HEADER] + [0] * 7
    assert (out.cpu().numpy()[:total] == expected_output(store, offs, total, set(range(1, 8)))).all()


def test_the_writers_refusals(gpu, store):
    w = keep(ArchiveWriter(gpu))
    images = store["images"]
    offs = offsets_at_residue(images, 0)
    arena = dev(place(images, offs))
    dst = torch.full((sum(len(i) for i in images),), 0xC3, dtype=torch.uint8, device="cuda")
    n = w.append(arena, offs[:7], [len(i) for i in images[:7]], dst)
    with pytest.raises(LongtailHipError) as e:
        w.finish(store["si"], store["vi"])
    assert e.value.code == errno.EINVAL, "seven blocks appended, the StoreIndex has eight"
    short = header_bytes(store["counts"][7], store["tags"][7]) - 1
    w.append(arena, offs[7:], [short], dst[n:])
    with pytest.raises(LongtailHipError) as e:
        w.finish(store["si"], store["vi"])
    assert e.value.code == errno.EINVAL, "the last image is below its block's header size"
    gpu.sync()
    w2 = keep(ArchiveWriter(gpu))
    assert w2.append(arena, offs, [len(i) for i in images], dst) == len(dst)
    gpu.sync()
    index = w2.finish(store["si"], store["vi"])
    body = dst.cpu().numpy()
    assert (body == np.concatenate(images)).all()
    a = keep(Archive(index, len(body)))
    rs, roffs, total, out = session(gpu, a)
    assert feed(rs, a, body, 0, len(body), out) == (8, len(body))
    assert rs.finish()[0] == 0 and (out.cpu().numpy()[:total] == expected_output(store, roffs, total)).all()
