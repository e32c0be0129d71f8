"""-m gpu: the two ingest sessions writing every block as its tag says (LTHIP_CODEC_BY_TAG) and writing raw blocks (LTHIP_CODEC_NONE),
on the trees of tests/test_gpu_ingest_stream.py, against the reference (oracle/_ref):

  * tag 0 for the whole tree, codec "none": VersionIndex == Longtail_CreateVersionIndex with tag 0, StoreIndex ==
    Longtail_CreateMissingContent, the images of all calls are the StoreIndex's blocks and each is byte for byte the reference's
    serialized stored block of its chunks (tests/test_gpu_raw_blocks.py: ref_raw_image); compressed_bytes == raw_bytes
  * tags rotating by top-level directory over {0, 'lz42', 'ztd2', 'ztd4'}, codec "by-tag": both indexes the reference's for those tags,
    stream == one-shot, every image with a tag opens through refh_open_stored_block -- which decodes with the codec THE TAG names --
    and every tag-0 image is byte-identical as above
  * the same with an lthip_store attached that holds half of the version's chunks
  * refusals: "by-tag" with a tag that names no codec here is ENOTSUP, "none" with a tag other than 0 EINVAL, from stream create and
    from the one-shot index (create, for cfg.compression_type); context and session work afterwards
  * codec "lz4" with tag 'lz42' and codec "by-tag" with the same tag give the same indexes and the same image bytes
  * the one-shot session by tag in several codec batches: indexes, compressed sizes and the last batch's images are the one-batch session's

The expected VersionIndex for per-asset tags is the reference's for ONE tag with its chunk-tag column replaced: a unique chunk carries
the tag of the asset it is first seen in (src/longtail.c:2951-2970); the harness of oracle/ passes one tag to Longtail_CreateVersionIndex.
Every comparison is equality."""
import ctypes as C
import errno

import numpy as np
import pytest
import torch

from longtail_amd.lib import Ingest, IngestStream, LongtailHipError, Store
from tests.gpu_util import dev_u64
from tests.test_gpu_ingest import parse_store_index, ref_missing_content, version_unique_lists
from tests.test_gpu_ingest_stream import _sessions, chunk_jobs, expected_of, index_buffers, open_stream, run_stream, slices_of, stream_tree, tree_of
from tests.test_gpu_raw_blocks import ref_opens_raw_image, ref_raw_image

pytestmark = pytest.mark.gpu

LZ4, ZTD2, ZTD4, BTL0 = 0x6C7A3432, 0x7A746432, 0x7A746434, 0x62746C30
CONFIGS = [(1024, 262144, 16), (4096, 1 << 20, 64)]
_open = []


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    """Sessions (those the stream suite's helpers opened too), then stores, are closed when the test ends: none may outlive its context."""
    yield
    while _sessions:
        _sessions.pop().close()
    while _open:
        _open.pop().close()


def keep(obj):
    _open.append(obj)
    return obj


def rotating_tags(tree, over):
    dirs = sorted({p.split("/")[0] for p in tree["paths"]})
    return np.array([over[dirs.index(p.split("/")[0]) % len(over)] for p in tree["paths"]], np.uint32)


def expected_version_index(oracle, ref, target, asset_tags, max_block, max_chunks):
    """The reference's VersionIndex of the tree with these per-asset tags (see the module's docstring)."""
    vi = bytearray(expected_of(oracle, ref, target, 0, max_block, max_chunks)[0])
    h = np.frombuffer(bytes(vi[:24]), np.uint32)
    na, nu, ni = int(h[3]), int(h[4]), int(h[5])
    assert na == len(asset_tags)
    o = 24 + na * 24
    counts = np.frombuffer(bytes(vi[o : o + na * 4]), np.uint32)
    starts = np.frombuffer(bytes(vi[o + na * 4 : o + na * 8]), np.uint32)
    idx = np.frombuffer(bytes(vi[o + na * 8 : o + na * 8 + ni * 4]), np.uint32)
    tags = np.zeros(nu, np.uint32)
    seen = np.zeros(nu, bool)
    for a in range(na):
        for u in idx[int(starts[a]) : int(starts[a]) + int(counts[a])]:
            if not seen[u]:
                seen[u] = True
                tags[u] = asset_tags[a]
    assert seen.all()
    t0 = o + na * 8 + ni * 4 + nu * 12
    vi[t0 : t0 + nu * 4] = tags.tobytes()
    return bytes(vi)


def run_one_shot(gpu, tree, target, codec, max_block, max_chunks, tag, asset_tags=None, store=None, ing=None, batch_bytes=0):
    """lthip_ingest_index / _write / _finish over the whole tree.  -> both indexes, the result, the images, the slice's host copies (in
    the shape of run_stream's result: one call, one slice)."""
    njobs, part = tree["part"].job_count, tree["part"]
    sl = chunk_jobs(gpu, tree, target, 0, njobs)
    if ing is None:
        ing = keep(Ingest(gpu, target, max_block, max_chunks, codec, compression_type=tag, batch_bytes=batch_bytes))
    if store is not None:
        ing.set_store(store)
    job_first = sl["d_first"].cpu().numpy().view(np.uint32).astype(np.uint64)
    t, _ = Ingest.tree(tree["sizes"].copy(), tree["offs"].copy(), tree["perms"].copy(), tree["path_data"], part.job_asset.copy(), job_first,
                       asset_tags=None if asset_tags is None else asset_tags.copy())
    vi, si = index_buffers(gpu, tree, sl["total"])
    ing.index(t, sl["d_hash"], sl["d_len"], sl["total"], sl["d_off"], sl["d_first"], sl["total"], vi)
    arena = torch.full((96 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    ing.write(sl["dev"], arena)
    res = ing.finish(si)
    first, offs, sizes = ing.images()
    host = arena.cpu().numpy()
    n = sl["total"]
    slices = [dict(data=sl["dev"].cpu().numpy(), off=sl["d_off"].cpu().numpy().view(np.uint64)[:n].copy(),
                   len=sl["d_len"].cpu().numpy().view(np.uint32)[:n].copy(), hash=sl["d_hash"].cpu().numpy().view(np.uint64)[:n].copy())]
    return dict(ing=ing, res=res, vi=bytes(vi.numpy()[: res.version_index_size]), si=bytes(si.numpy()[: res.store_index_size]),
                calls=[(first, [host[int(o) : int(o) + int(k)].copy() for o, k in zip(offs, sizes)])], slices=slices,
                comp=ing.compressed_sizes(res.blocks))


def check_images_by_tag(gpu, ref, run):
    """call order == StoreIndex order; a tag-0 image is the reference's serialized stored block of its chunks, byte for byte, and opens
    with Longtail_ReadStoredBlockFromBuffer; every other image opens through the reference's reader and the codec its TAG names and
    decodes to the chunks' bytes.  -> (blocks holding chunks of more than one slice, of those the raw ones, the tags met, payload bytes)"""
    si = parse_store_index(run["si"])
    where, slice_of = {}, {}
    for k, sl in enumerate(run["slices"]):
        for o, n, h in zip(sl["off"], sl["len"], sl["hash"]):
            if int(h) not in where:
                where[int(h)] = sl["data"][int(o) : int(o) + int(n)]
                slice_of[int(h)] = k
    nxt, images = 0, []
    for first, imgs in run["calls"]:
        assert first == nxt, "first_block of a call continues where the call before ended"
        nxt += len(imgs)
        images += imgs
    assert len(images) == run["res"].blocks == len(si["block_hashes"])
    mixed = mixed_raw = stored = 0
    for b, image in enumerate(images):
        c0, n = int(si["block_offsets"][b]), int(si["block_counts"][b])
        h = np.ascontiguousarray(si["chunk_hashes"][c0 : c0 + n])
        s = np.ascontiguousarray(si["chunk_sizes"][c0 : c0 + n])
        raw = int(s.astype(np.int64).sum())
        tag = int(si["block_tags"][b])
        content = np.concatenate([where[int(x)] for x in h])
        assert int(np.frombuffer(image[:8].tobytes(), np.uint64)[0]) == int(si["block_hashes"][b]), b
        several = len({slice_of[int(x)] for x in h}) > 1
        if tag == 0:
            expect = ref_raw_image(ref, h, s, content)
            assert len(image) == len(expect) == gpu.block_index_size(n) + raw, b
            assert (image == expect).all(), (b, n, int(np.flatnonzero(image != expect)[0]))
            assert ref_opens_raw_image(ref, image) == raw, b
            stored += raw
            mixed_raw += several
        else:
            out = np.zeros(raw + 8, np.uint8)
            got = C.c_uint64(0)
            err = ref.dll.refh_open_stored_block(image.ctypes.data, len(image), n, h.ctypes.data, s.ctypes.data, tag, out.ctypes.data, raw, C.byref(got))
            assert err == 0, (b, hex(tag), err)
            assert got.value == raw and (out[:raw] == content).all(), b
            stored += len(image) - int(gpu.lib.dll.lthip_stored_block_header_size(n))
        mixed += several
    return mixed, mixed_raw, set(int(t) for t in si["block_tags"]), stored


# ---- tag 0 for the whole tree, codec "none" ----


@pytest.mark.parametrize("cut", ["one", "per-job", "one-shot"])
@pytest.mark.parametrize("target,max_block,max_chunks", CONFIGS)
def test_a_tree_of_raw_blocks_is_the_references(gpu, oracle, ref, target, max_block, max_chunks, cut):
    tree = tree_of(oracle, ref, target)
    expect_vi, expect_si, unique_bytes = expected_of(oracle, ref, target, 0, max_block, max_chunks)
    if cut == "one-shot":
        run = run_one_shot(gpu, tree, target, "none", max_block, max_chunks, None)
    else:
        run = run_stream(gpu, tree, target, "none", max_block, max_chunks, None, slices_of(cut, tree["part"].job_count))
    assert run["vi"] == expect_vi, "VersionIndex differs from Longtail_CreateVersionIndex with tag 0"
    assert run["si"] == expect_si, "StoreIndex differs from Longtail_CreateMissingContent"
    res = run["res"]
    mixed, mixed_raw, tags, stored = check_images_by_tag(gpu, ref, run)
    assert tags == {0}
    assert res.raw_bytes == unique_bytes == res.compressed_bytes == stored
    assert res.gathered_blocks == 0 and res.gathered_bytes == 0, "raw blocks never go through the block assembly"
    if cut == "one-shot":
        assert (run["comp"] == [len(i) - gpu.block_index_size(int(np.frombuffer(i[12:16].tobytes(), np.uint32)[0])) for i in run["calls"][0][1]]).all()
    if cut == "per-job":  # (about this test's own input: the carry buffer feeds a raw image)
        assert mixed_raw > 0, "no raw block holds chunks of two slices"


# ---- mixed tags, codec "by-tag" ----


@pytest.mark.parametrize("cut", ["one", "per-job"])
@pytest.mark.parametrize("target,max_block,max_chunks", CONFIGS)
def test_every_block_is_written_as_its_tag_says(gpu, oracle, ref, target, max_block, max_chunks, cut):
    tree = tree_of(oracle, ref, target)
    tags = rotating_tags(tree, (0, LZ4, ZTD2, ZTD4))
    expect_vi = expected_version_index(oracle, ref, target, tags, max_block, max_chunks)
    uh, us, ut = version_unique_lists(expect_vi)
    expect_si = ref_missing_content(ref, np.zeros(0, np.uint64), uh, us, ut, max_block, max_chunks)
    one = run_one_shot(gpu, tree, target, "by-tag", max_block, max_chunks, None, asset_tags=tags)
    run = run_stream(gpu, tree, target, "by-tag", max_block, max_chunks, None, slices_of(cut, tree["part"].job_count), asset_tags=tags.copy())
    for name, r in (("one-shot", one), ("stream", run)):
        assert r["vi"] == expect_vi, f"{name}: VersionIndex differs from the reference's for these tags"
        assert r["si"] == expect_si, f"{name}: StoreIndex differs from Longtail_CreateMissingContent over the VersionIndex's unique lists"
        mixed, _, met, stored = check_images_by_tag(gpu, ref, r)
        assert len(met) >= 3 and 0 in met, met
        assert r["res"].compressed_bytes == stored
    assert (run["res"].blocks, run["res"].raw_bytes, run["res"].unique_local) == (one["res"].blocks, one["res"].raw_bytes, one["res"].unique_local)


# ---- the one-shot session, by tag, in more than one codec batch ----

SMALL_BATCH = 1 << 20


def last_batch_start(raw_sizes, batch_bytes):
    """Where lthip_ingest_write's last batch begins when the arena is no limit: a batch takes blocks until the next one would bring its
    raw bytes above batch_bytes, and always at least one."""
    b0 = acc = 0
    for b, raw in enumerate(raw_sizes):
        if b > b0 and acc + raw > batch_bytes:
            b0, acc = b, 0
        acc += raw
    return b0


@pytest.mark.parametrize("rotate_by", ["directory", "asset"])
def test_by_tag_in_several_batches_writes_what_one_batch_writes(gpu, oracle, ref, rotate_by):
    """A one-shot session that writes by tag in more than one batch: the block hashes, the compressed sizes, the tags and the scatter of
    the codec calls' sizes of a batch all start at a block above 0.  Same indexes (the reference's), same compressed sizes of all blocks,
    and the last batch's images are byte for byte those of the same blocks written in one batch.

    The tags rotate over (0, 'lz42', 'ztd2', 'ztd4') by top-level directory, as in the tests above, and by asset.  By directory the tree's
    blocks are four runs of one tag each, the tag-0 run first, and a last batch is a tail of the blocks no larger than the batches
    before it: whatever the batch size it holds no tag-0 block and no codec's blocks with another's in between.  By asset it does, at
    the 1 MiB of tests/test_gpu_ingest.py's packing-in-slices test: the conditions on the last batch are asserted for that case."""
    target, max_block, max_chunks = CONFIGS[0]
    tree = tree_of(oracle, ref, target)
    over = (0, LZ4, ZTD2, ZTD4)
    tags = rotating_tags(tree, over) if rotate_by == "directory" else np.array([over[a % len(over)] for a in range(len(tree["paths"]))], np.uint32)
    expect_vi = expected_version_index(oracle, ref, target, tags, max_block, max_chunks)
    uh, us, ut = version_unique_lists(expect_vi)
    expect_si = ref_missing_content(ref, np.zeros(0, np.uint64), uh, us, ut, max_block, max_chunks)
    once = run_one_shot(gpu, tree, target, "by-tag", max_block, max_chunks, None, asset_tags=tags)
    small = run_one_shot(gpu, tree, target, "by-tag", max_block, max_chunks, None, asset_tags=tags, batch_bytes=SMALL_BATCH)
    # ---- about this test's own input, read off the one-batch run's StoreIndex: the small run's last batch starts above block 0 and holds
    # blocks of two codecs (a tag is a codec key here); by asset also a raw block, and one codec's blocks with another block in between ----
    si = parse_store_index(once["si"])
    raw = [int(si["chunk_sizes"][int(o) : int(o) + int(n)].astype(np.int64).sum()) for o, n in zip(si["block_offsets"], si["block_counts"])]
    b0 = last_batch_start(raw, SMALL_BATCH)
    last = [int(t) for t in si["block_tags"][b0:]]
    assert 0 < b0 < len(raw)
    assert len(set(last) - {0}) >= 2, [hex(t) for t in last]
    if rotate_by == "asset":
        assert 0 in last, [hex(t) for t in last]
        assert any(np.diff(np.flatnonzero(np.array(last) == t)).max(initial=1) > 1 for t in set(last) - {0}), "every codec's blocks are one run"
    assert once["res"].gathered_blocks > 0
    # ---- what the issue is about ----
    for name, r in (("one batch", once), ("small batches", small)):
        assert r["vi"] == expect_vi, f"{name}: VersionIndex differs from the reference's for these tags"
        assert r["si"] == expect_si, f"{name}: StoreIndex differs from Longtail_CreateMissingContent over the VersionIndex's unique lists"
    assert small["res"].blocks == once["res"].blocks == len(raw) and (small["comp"] == once["comp"]).all()
    assert (small["res"].compressed_bytes, small["res"].gathered_blocks, small["res"].gathered_bytes) == \
        (once["res"].compressed_bytes, once["res"].gathered_blocks, once["res"].gathered_bytes)
    (first_once, all_images), (first, images) = once["calls"][0], small["calls"][0]
    assert first_once == 0 and len(all_images) == len(raw), "the default batch size takes the tree in one batch"
    assert first == b0 and len(images) == len(raw) - b0, "the last batch is not the one this test reckoned with"
    for b, image in enumerate(images, b0):
        assert len(image) == len(all_images[b]) and (image == all_images[b]).all(), b


# ---- with a store attached ----


def test_by_tag_into_a_store_that_holds_half_of_the_version(gpu, oracle, ref):
    target, max_block, max_chunks = CONFIGS[0]
    tree = tree_of(oracle, ref, target)
    tags = rotating_tags(tree, (0, LZ4, ZTD2, ZTD4))
    expect_vi = expected_version_index(oracle, ref, target, tags, max_block, max_chunks)
    uh, us, ut = version_unique_lists(expect_vi)
    holds = uh[::2].copy()
    store = keep(Store(gpu, 0))
    store.add(dev_u64(holds))
    expect_si = ref_missing_content(ref, holds, uh, us, ut, max_block, max_chunks)
    # the stream session, cut per job
    st = open_stream(gpu, stream_tree(tree, tags.copy()), target, max_block, max_chunks, "by-tag")
    st.set_store(store)
    calls, slices, chunks_all = [], [], 0
    for first_job, count in slices_of("per-job", tree["part"].job_count):
        sl = chunk_jobs(gpu, tree, target, first_job, count)
        arena = torch.zeros(max(64, st.arena_bound(sl["bytes"], sl["total"])), dtype=torch.uint8, device="cuda")
        st.slice(first_job, count, sl["dev"], sl["d_off"], sl["d_len"], sl["d_hash"], sl["d_first"], sl["total"], arena)
        first, offs, sizes = st.images()
        host = arena.cpu().numpy()
        calls.append((first, [host[int(o) : int(o) + int(k)].copy() for o, k in zip(offs, sizes)]))
        n = sl["total"]
        slices.append(dict(data=sl["dev"].cpu().numpy(), off=sl["d_off"].cpu().numpy().view(np.uint64)[:n].copy(),
                           len=sl["d_len"].cpu().numpy().view(np.uint32)[:n].copy(), hash=sl["d_hash"].cpu().numpy().view(np.uint64)[:n].copy()))
        chunks_all += n
    arena = torch.zeros(st.arena_bound(0, 0), dtype=torch.uint8, device="cuda")
    vi, si = index_buffers(gpu, tree, chunks_all)
    res = st.finish(arena, vi, si)
    first, offs, sizes = st.images()
    host = arena.cpu().numpy()
    calls.append((first, [host[int(o) : int(o) + int(k)].copy() for o, k in zip(offs, sizes)]))
    run = dict(res=res, vi=bytes(vi.numpy()[: res.version_index_size]), si=bytes(si.numpy()[: res.store_index_size]), calls=calls, slices=slices)
    one = run_one_shot(gpu, tree, target, "by-tag", max_block, max_chunks, None, asset_tags=tags, store=store)
    for name, r in (("stream", run), ("one-shot", one)):
        assert r["vi"] == expect_vi, name
        assert r["si"] == expect_si, f"{name}: StoreIndex differs from Longtail_CreateMissingContent(store, version)"
        _, _, met, stored = check_images_by_tag(gpu, ref, r)
        assert len(met) >= 3 and 0 in met
        assert 0 < r["res"].unique_local < r["res"].unique_all and r["res"].compressed_bytes == stored


# ---- refusals ----


def test_tags_the_codec_mode_does_not_take_are_refused(gpu, oracle, ref):
    target, max_block, max_chunks = CONFIGS[0]
    tree = tree_of(oracle, ref, target)
    njobs, part = tree["part"].job_count, tree["part"]
    bad = rotating_tags(tree, (0, LZ4, BTL0))
    zeros = np.zeros(len(bad), np.uint32)
    # ---- the stream session: from create ----
    for codec, ctype, atags, code in (("by-tag", None, bad, errno.ENOTSUP), ("by-tag", BTL0, None, errno.ENOTSUP), ("none", None, bad, errno.EINVAL),
                                      ("none", LZ4, None, errno.EINVAL), ("none", LZ4, zeros, errno.EINVAL)):
        with pytest.raises(LongtailHipError) as e:
            IngestStream(gpu, stream_tree(tree, None if atags is None else atags.copy()), target, max_block, max_chunks, codec, compression_type=ctype)
        assert e.value.code == code, (codec, ctype, code)
    # ---- the one-shot session: cfg.compression_type from create, the asset tags from index; the session works afterwards ----
    for codec, ctype, code in (("by-tag", BTL0, errno.ENOTSUP), ("none", ZTD2, errno.EINVAL)):
        with pytest.raises(LongtailHipError) as e:
            Ingest(gpu, target, max_block, max_chunks, codec, compression_type=ctype)
        assert e.value.code == code
    sl = chunk_jobs(gpu, tree, target, 0, njobs)
    job_first = sl["d_first"].cpu().numpy().view(np.uint32).astype(np.uint64)
    for codec, good_tags, code in (("by-tag", rotating_tags(tree, (0, LZ4, ZTD2, ZTD4)), errno.ENOTSUP), ("none", zeros, errno.EINVAL)):
        ing = keep(Ingest(gpu, target, max_block, max_chunks, codec, compression_type=0))
        t, _ = Ingest.tree(tree["sizes"].copy(), tree["offs"].copy(), tree["perms"].copy(), tree["path_data"], part.job_asset.copy(), job_first,
                           asset_tags=bad.copy())
        vi, _ = index_buffers(gpu, tree, sl["total"])
        with pytest.raises(LongtailHipError) as e:
            ing.index(t, sl["d_hash"], sl["d_len"], sl["total"], sl["d_off"], sl["d_first"], sl["total"], vi)
        assert e.value.code == code
        run = run_one_shot(gpu, tree, target, codec, max_block, max_chunks, 0, asset_tags=good_tags, ing=ing)  # the same session, good tags
        expect_vi = expected_version_index(oracle, ref, target, good_tags, max_block, max_chunks)
        assert run["vi"] == expect_vi
        uh, us, ut = version_unique_lists(expect_vi)
        assert run["si"] == ref_missing_content(ref, np.zeros(0, np.uint64), uh, us, ut, max_block, max_chunks)
        check_images_by_tag(gpu, ref, run)
    with pytest.raises(ValueError):  # the wrapper: "by-tag" has no default tag
        IngestStream(gpu, stream_tree(tree), target, max_block, max_chunks, "by-tag")


# ---- unchanged behaviour ----


@pytest.mark.parametrize("cut", ["one", "one-shot"])
def test_one_codec_and_by_tag_agree_on_a_tree_of_that_tag(gpu, oracle, ref, cut):
    target, max_block, max_chunks = CONFIGS[0]
    tree = tree_of(oracle, ref, target)
    runs = []
    for codec in ("lz4", "by-tag"):
        if cut == "one-shot":
            runs.append(run_one_shot(gpu, tree, target, codec, max_block, max_chunks, LZ4))
        else:
            runs.append(run_stream(gpu, tree, target, codec, max_block, max_chunks, LZ4, slices_of(cut, tree["part"].job_count)))
    a, b = runs
    expect_vi, expect_si, _ = expected_of(oracle, ref, target, LZ4, max_block, max_chunks)
    assert a["vi"] == b["vi"] == expect_vi and a["si"] == b["si"] == expect_si
    ia, ib = ([i for _, imgs in r["calls"] for i in imgs] for r in (a, b))
    assert len(ia) == len(ib) == a["res"].blocks > 0
    assert all(len(x) == len(y) and (x == y).all() for x, y in zip(ia, ib))
    assert a["res"].compressed_bytes == b["res"].compressed_bytes and a["res"].gathered_blocks == b["res"].gathered_blocks
