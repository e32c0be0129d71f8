"""-m gpu: the ingest sessions against a store that already has content (lthip_store attached with lthip_ingest_stream_set_store /
lthip_ingest_set_store), against the reference run on the same tree (oracle/_ref):

  * serialized VersionIndex == Longtail_CreateVersionIndex + Longtail_WriteVersionIndexToBuffer: the whole version's, store or not
  * serialized StoreIndex   == Longtail_CreateMissingContent(existing, version) + Longtail_WriteStoreIndexToBuffer, whatever the cuts:
      (a) no store / an empty store    -> the StoreIndex of today (everything is missing)
      (b) every chunk of the version   -> the 16-byte header, no images
      (c) every third unique chunk, 1 000 unrelated hashes, 0 and 0xFFFF...FFFF
      (d) the previous version, added with lthip_store_add_index from the StoreIndex its own session produced
  * the images of all calls, in call order, are the StoreIndex's blocks; each opens with Longtail_ReadStoredBlockFromBuffer and
    decodes with the reference codec to its chunks' bytes
  * the one-shot session the same at world 1, and at world 2 (two sessions on one GPU fed the job-ordered arrays): each rank's
    StoreIndex is the reference's with existing = store + the other rank's chunks, the ranks' written sets partition what is missing

Every comparison is equality."""
import ctypes as C
import errno

import numpy as np
import pytest
import torch

from longtail_amd.dist import JobPartition
from longtail_amd.lib import Ingest, IngestStream, LongtailHipError, Store
from tests.gpu_util import dev_u64
from tests.test_gpu_ingest import check_images as check_one_shot_images
from tests.test_gpu_ingest import make_files, parse_store_index, rank_session, ref_missing_content, version_unique_lists
from tests.test_gpu_ingest_stream import CONFIGS, chunk_jobs, expected_of, index_buffers, slices_of, stream_tree, tree_of

pytestmark = pytest.mark.gpu

EMPTY = 0xFFFFFFFFFFFFFFFF
# one LZ4 and one zstd configuration of the stream suite, each with the smallest max_block_size there: blocks close often
STORE_CONFIGS = [min((c for c in CONFIGS if c[1] == codec), key=lambda c: c[2]) for codec in ("lz4", "zstd")]
CUTS = ["one", "per-job", "random"]
KINDS = ["none", "empty", "all", "third"]
_open = []


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    """Sessions, then stores, are closed when the test ends, passed or failed: neither may outlive its context."""
    yield
    while _open:
        _open.pop().close()


def keep(obj):
    _open.append(obj)
    return obj


def cuts_of(kind, njobs):
    if kind != "random":
        return slices_of(kind, njobs)
    rng = np.random.default_rng(njobs)
    inner = np.sort(rng.choice(np.arange(1, njobs), size=min(5, njobs - 1), replace=False)).tolist()
    bounds = [0] + inner + [njobs]
    return [(a, b - a) for a, b in zip(bounds[:-1], bounds[1:])]


def tag_of(ref, codec):
    return ref.lz4_type if codec == "lz4" else ref.zstd_default


def store_of(gpu, kind, uh):
    """-> (the store or None, the hashes it holds as the reference's `existing`)"""
    none = np.zeros(0, np.uint64)
    if kind == "none":
        return None, none
    store = keep(Store(gpu, 0))
    if kind == "empty":
        return store, none
    if kind == "all":
        holds = uh.copy()
    else:
        unrelated = np.random.default_rng(4).integers(1, 2**64 - 1, size=1_000, dtype=np.uint64)
        assert not np.isin(unrelated, uh).any()
        holds = np.concatenate([uh[::3], unrelated, np.array([0, EMPTY], np.uint64)])
    store.add(dev_u64(holds))
    return store, holds


def run_stream(gpu, tree, target, codec, max_block, max_chunks, tag, cuts, store, late_set_store=False):
    """The session over the given cuts with `store` attached (None: never attached).  -> both indexes, the result, the store stats, per
    call the image bytes, per slice the host copies of its data and lists."""
    st = keep(IngestStream(gpu, stream_tree(tree), target, max_block, max_chunks, codec, compression_type=tag))
    if store is not None:
        st.set_store(store)
    calls, slices, chunks_all = [], [], 0

    def take(arena):
        first, offs, sizes = st.images()
        host = arena.cpu().numpy()
        calls.append((first, [host[int(o) : int(o) + int(n)].copy() for o, n in zip(offs, sizes)]))

    for k, (first_job, count) in enumerate(cuts):
        sl = chunk_jobs(gpu, tree, target, first_job, count)
        arena = torch.zeros(max(64, st.arena_bound(sl["bytes"], sl["total"])), dtype=torch.uint8, device="cuda")
        st.slice(first_job, count, sl["dev"], sl["d_off"], sl["d_len"], sl["d_hash"], sl["d_first"], sl["total"], arena)
        take(arena)
        if late_set_store and k == 0:  # refused once a slice has been taken, whatever the store; the session goes on as it was
            for late in (store, None):
                with pytest.raises(LongtailHipError) as e:
                    st.set_store(late)
                assert e.value.code == errno.EINVAL
        n = sl["total"]
        slices.append(dict(data=sl["dev"].cpu().numpy(), off=sl["d_off"].cpu().numpy().view(np.uint64)[:n].copy(),
                           len=sl["d_len"].cpu().numpy().view(np.uint32)[:n].copy(), hash=sl["d_hash"].cpu().numpy().view(np.uint64)[:n].copy()))
        chunks_all += n
    arena = torch.zeros(st.arena_bound(0, 0), dtype=torch.uint8, device="cuda")
    vi, si = index_buffers(gpu, tree, chunks_all)
    res = st.finish(arena, vi, si)
    take(arena)
    return dict(st=st, res=res, stats=st.store_stats(), vi=bytes(vi.numpy()[: res.version_index_size]), si=bytes(si.numpy()[: res.store_index_size]),
                calls=calls, slices=slices)


def check_stream(gpu, ref, run, expect_vi, expect_si, existing):
    """Both indexes are the reference's; the images of all calls are the StoreIndex's blocks and decode to its chunks' bytes; result and
    store stats agree with the parsed StoreIndex.  -> blocks that hold chunks of more than one slice call"""
    assert run["vi"] == expect_vi, "VersionIndex differs from Longtail_CreateVersionIndex"
    assert run["si"] == expect_si, "StoreIndex differs from Longtail_CreateMissingContent(store, version)"
    uh, us, _ = version_unique_lists(expect_vi)
    si = parse_store_index(run["si"])
    res = run["res"]
    held = np.isin(uh, existing)
    assert (si["chunk_hashes"] == uh[~held]).all() and (si["chunk_sizes"] == us[~held]).all()
    assert res.unique_all == len(uh) and res.unique_local == len(si["chunk_hashes"]) and res.chunks_local == res.chunks_all
    assert res.raw_bytes == int(si["chunk_sizes"].astype(np.int64).sum()) and res.blocks == len(si["block_hashes"])
    assert res.version_index_size == len(expect_vi) and res.store_index_size == len(expect_si)
    assert run["stats"] == (int(held.sum()), int(us[held].astype(np.int64).sum()))
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
    assert len(images) == res.blocks
    mixed, compressed = 0, 0
    for b, image in enumerate(images):
        c0, n = int(si["block_offsets"][b]), int(si["block_counts"][b])
        h = np.ascontiguousarray(si["chunk_hashes"][c0 : c0 + n])
        s = np.ascontiguousarray(si["chunk_sizes"][c0 : c0 + n])
        raw = int(s.astype(np.int64).sum())
        assert int(np.frombuffer(image[:8].tobytes(), np.uint64)[0]) == int(si["block_hashes"][b]), b
        out = np.zeros(raw + 8, np.uint8)
        got = C.c_uint64(0)
        err = ref.dll.refh_open_stored_block(image.ctypes.data, len(image), n, h.ctypes.data, s.ctypes.data, int(si["block_tags"][b]),
                                             out.ctypes.data, raw, C.byref(got))
        assert err == 0, (b, err)
        assert got.value == raw and (out[:raw] == np.concatenate([where[int(x)] for x in h])).all(), b
        mixed += len({slice_of[int(x)] for x in h}) > 1
        compressed += len(image) - int(gpu.lib.dll.lthip_stored_block_header_size(n))
    assert res.compressed_bytes == compressed
    return mixed


def assert_not_trivial(run, cut, mixed):
    """About the test's own input: some chunks are written and some are not, a block is assembled from more than one byte range, and
    under per-job cuts a block holds chunks of two slice calls."""
    res = run["res"]
    assert 0 < res.unique_local < res.unique_all
    assert res.gathered_blocks > 0
    if cut == "per-job":
        assert mixed > 0, "no block holds chunks of two slice calls"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("target,codec,max_block,max_chunks", STORE_CONFIGS)
def test_stream_session_writes_what_the_store_lacks(gpu, oracle, ref, target, codec, max_block, max_chunks, cut, kind):
    tree = tree_of(oracle, ref, target)
    tag = tag_of(ref, codec)
    expect_vi, today_si, _ = expected_of(oracle, ref, target, tag, max_block, max_chunks)
    uh, us, ut = version_unique_lists(expect_vi)
    store, existing = store_of(gpu, kind, uh)
    expect_si = ref_missing_content(ref, existing, uh, us, ut, max_block, max_chunks)
    run = run_stream(gpu, tree, target, codec, max_block, max_chunks, tag, cuts_of(cut, tree["part"].job_count), store,
                     late_set_store=kind == "third")
    mixed = check_stream(gpu, ref, run, expect_vi, expect_si, existing)
    if kind in ("none", "empty"):
        assert run["si"] == today_si and run["res"].unique_local == run["res"].unique_all and run["stats"] == (0, 0)
    elif kind == "all":
        assert len(run["si"]) == 16 and np.frombuffer(run["si"], np.uint32).tolist() == [1 << 24, 0, 0, 0]
        assert all(len(imgs) == 0 for _, imgs in run["calls"]) and run["res"].blocks == 0 and run["res"].compressed_bytes == 0
        assert run["stats"][0] == run["res"].unique_all
    else:
        assert_not_trivial(run, cut, mixed)


_versions = {}


def next_version(oracle, ref, target):
    """Tree B of test (d): tree A with 1 000 bytes inserted in the middle of two files, one file dropped and one added."""
    if target not in _versions:
        files = [(n, d) for n, d in make_files(oracle, target) if n != "dir2/sub1/file05.bin"]
        assert len(files) == len(make_files(oracle, target)) - 1
        for name, seed in (("dir1/sub1/file01.bin", 201), ("dir1/sub0/file10.bin", 202)):
            i = [n for n, _ in files].index(name)
            d = files[i][1]
            files[i] = (name, np.concatenate([d[: len(d) // 2], oracle.synth(1_000, seed, 0), d[len(d) // 2 :]]))
        files.append(("dir1/added.bin", oracle.synth(300_000, 203, 1)))
        paths, sizes, offs, perms, path_data = ref.tree_file_infos(files)
        _versions[target] = dict(files=files, by_name=dict(files), paths=paths, sizes=sizes, offs=offs, perms=perms, path_data=path_data,
                                 part=JobPartition(sizes, target, 1, "range"))
    return _versions[target]


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("target,codec,max_block,max_chunks", STORE_CONFIGS)
def test_the_next_version_into_a_store_that_holds_the_one_before(gpu, oracle, ref, target, codec, max_block, max_chunks, cut):
    tag = tag_of(ref, codec)
    tree_a, tree_b = tree_of(oracle, ref, target), next_version(oracle, ref, target)
    vi_a, si_a, _ = expected_of(oracle, ref, target, tag, max_block, max_chunks)
    store = keep(Store(gpu, 0))
    run_a = run_stream(gpu, tree_a, target, codec, max_block, max_chunks, tag, cuts_of(cut, tree_a["part"].job_count), store)
    assert run_a["vi"] == vi_a and run_a["si"] == si_a and run_a["stats"] == (0, 0)
    store.add_index(run_a["si"])  # what the session wrote is what the store holds now
    uh_a = version_unique_lists(vi_a)[0]
    assert store.added == len(uh_a) == store.distinct
    key = ("b", target, tag)
    if key not in _versions:
        _versions[key] = ref.version_index(tree_b["files"], target, 0, tag)[0]
    vi_b = _versions[key]
    uh, us, ut = version_unique_lists(vi_b)
    expect_si = ref_missing_content(ref, uh_a, uh, us, ut, max_block, max_chunks)
    run_b = run_stream(gpu, tree_b, target, codec, max_block, max_chunks, tag, cuts_of(cut, tree_b["part"].job_count), store)
    mixed = check_stream(gpu, ref, run_b, vi_b, expect_si, uh_a)
    assert_not_trivial(run_b, cut, mixed)
    assert run_b["res"].unique_local < run_b["res"].unique_all // 4, "most of version B is in the store"


def one_shot(gpu, ref, files, target, world, rank, policy, codec, max_block, max_chunks, tag, lists, store, ing=None):
    """tests/test_gpu_ingest.py's rank_session with a store attached before lthip_ingest_index (`ing`: a session to run again; a store
    of None detaches the one it had)."""
    local = rank_session(gpu, ref, files, target, world, rank, policy, codec, max_block, max_chunks, tag)
    paths, sizes, offs, perms, path_data = local["infos"]
    part, mine, total = local["part"], local["mine"], local["total"]
    all_hash = torch.cat([lists[j][0] for j in range(part.job_count)])
    all_lens = torch.cat([lists[j][1] for j in range(part.job_count)])
    job_first = np.concatenate([[0], np.cumsum([int(lists[j][0].numel()) for j in range(part.job_count)])]).astype(np.uint64)
    n_all = int(job_first[-1])
    if ing is None:
        ing = keep(Ingest(gpu, target, max_block, max_chunks, codec, compression_type=tag))
        assert ing.store_stats() == (0, 0)
        if store is not None:
            ing.set_store(store)
    else:
        ing.set_store(store)
    tree, _ = Ingest.tree(sizes.copy(), offs.copy(), perms.copy(), path_data, part.job_asset.copy(), job_first.copy(),
                          my_jobs=None if world == 1 else mine.copy())
    vi = torch.zeros(gpu.lib.dll.lthip_version_index_size(len(sizes), n_all, n_all, len(path_data)) + 64, dtype=torch.uint8).pin_memory()
    ing.index(tree, all_hash, all_lens, n_all, local["d_off"], local["d_first"], total, vi if rank == 0 else None)
    arena = torch.zeros(96 << 20, dtype=torch.uint8, device="cuda")
    ing.write(local["dev"], arena)
    si = torch.zeros(16 + 32 * max(total, 1) + 64, dtype=torch.uint8).pin_memory()
    res = ing.finish(si)
    local.update(ing=ing, res=res, stats=ing.store_stats(), vi=bytes(vi.numpy()[: res.version_index_size]) if rank == 0 else None,
                 si=bytes(si.numpy()[: res.store_index_size]), arena=arena, comp=ing.compressed_sizes(res.blocks), all_hash=all_hash,
                 all_lens=all_lens)
    return local


def job_lists(probes):
    lists = {}
    for p in probes:
        for m, j in enumerate(p["mine"]):
            a, b = int(p["first"][m]), int(p["first"][m + 1])
            lists[int(j)] = (p["d_hash"][a:b].clone(), p["d_len"][a:b].clone())
    return lists


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("target,codec,max_block,max_chunks", STORE_CONFIGS)
def test_one_shot_session_writes_what_the_store_lacks(gpu, oracle, ref, target, codec, max_block, max_chunks, kind):
    tree = tree_of(oracle, ref, target)
    tag = tag_of(ref, codec)
    expect_vi, today_si, _ = expected_of(oracle, ref, target, tag, max_block, max_chunks)
    uh, us, ut = version_unique_lists(expect_vi)
    store, existing = store_of(gpu, kind, uh)
    files = tree["files"]
    lists = job_lists([rank_session(gpu, ref, files, target, 1, 0, "range", codec, max_block, max_chunks, tag)])
    sess = one_shot(gpu, ref, files, target, 1, 0, "range", codec, max_block, max_chunks, tag, lists, store)
    assert sess["vi"] == expect_vi, "VersionIndex differs from Longtail_CreateVersionIndex"
    assert sess["si"] == ref_missing_content(ref, existing, uh, us, ut, max_block, max_chunks), "StoreIndex differs from Longtail_CreateMissingContent"
    res, held = sess["res"], np.isin(uh, existing)
    assert res.unique_all == len(uh) and res.unique_local == int((~held).sum()) and res.raw_bytes == int(us[~held].astype(np.int64).sum())
    assert sess["stats"] == (int(held.sum()), int(us[held].astype(np.int64).sum()))
    assert res.compressed_bytes == int(sess["comp"].astype(np.int64).sum())
    check_one_shot_images(gpu, ref, sess, 0 if codec == "lz4" else 1, tag, max_block)
    if kind in ("none", "empty"):
        assert sess["si"] == today_si and sess["stats"] == (0, 0)
    elif kind == "all":
        assert len(sess["si"]) == 16 and res.blocks == 0 and res.unique_local == 0 and sess["stats"][0] == res.unique_all
    else:
        assert 0 < res.unique_local < res.unique_all and res.gathered_blocks > 0
    if kind == "third":  # detached again: the same session writes everything
        again = one_shot(gpu, ref, files, target, 1, 0, "range", codec, max_block, max_chunks, tag, lists, None, ing=sess["ing"])
        assert again["si"] == today_si and again["vi"] == expect_vi and again["stats"] == (0, 0)


@pytest.mark.parametrize("policy", ["range", "mod"])
def test_one_shot_sessions_of_two_ranks_partition_what_the_store_lacks(gpu, oracle, ref, policy):
    target, codec, max_block, max_chunks = STORE_CONFIGS[0]
    world, tag = 2, ref.lz4_type
    tree = tree_of(oracle, ref, target)
    files = tree["files"]
    expect_vi, _, _ = expected_of(oracle, ref, target, tag, max_block, max_chunks)
    uh, us, ut = version_unique_lists(expect_vi)
    store, existing = store_of(gpu, "third", uh)  # every rank holds the same store
    lists = job_lists([rank_session(gpu, ref, files, target, world, r, policy, codec, max_block, max_chunks, tag) for r in range(world)])
    sessions = [one_shot(gpu, ref, files, target, world, r, policy, codec, max_block, max_chunks, tag, lists, store) for r in range(world)]
    assert sessions[0]["vi"] == expect_vi, "rank 0's VersionIndex differs from the single-process reference"
    wrote = [parse_store_index(s["si"])["chunk_hashes"] for s in sessions]
    held = np.isin(uh, existing)
    allw = np.concatenate(wrote)
    assert len(allw) == int((~held).sum()) and set(allw.tolist()) == set(uh[~held].tolist())  # disjoint, and together what is missing
    assert all(len(w) > 0 for w in wrote)
    for r, s in enumerate(sessions):
        others = np.concatenate([existing, wrote[1 - r]])  # the store and the chunks first seen in the other rank's jobs
        assert s["si"] == ref_missing_content(ref, others, uh, us, ut, max_block, max_chunks), f"rank {r} StoreIndex"
        assert s["res"].unique_all == len(uh) and s["res"].unique_local == len(wrote[r])
        check_one_shot_images(gpu, ref, s, 0, tag, max_block)
    assert sum(s["stats"][0] for s in sessions) == int(held.sum())
    assert sum(s["stats"][1] for s in sessions) == int(us[held].astype(np.int64).sum())
