"""-m gpu: the device cache of decoded blocks (lthip_block_cache_*, lthip_restore_set_cache / from_cache / cache_stats;
include/longtail_hip.h "a cache of decoded blocks").

   1 a second session needs nothing: the clip sweep served wholly from what the first session left, verify on and off
   2 tagged stores (LZ4, zstd, by tag; every hash type the fixtures write them with): a full restore fills the cache, 64 random windows
     and a second full restore are served from it without a decoded byte
   3 mixed feeding: every second block cached, the rest delivered in one call and in three, from_cache before, between and after them;
     the same on a session from a base and on an update in place, with the in-place ordering refusals
   4 LRU against the Python model (tests/block_cache_util.py): two slots, three blocks, a scripted sequence of sessions
   5 pins: live sessions hold both slots, a third session's delivery is bypassed; once they finished the next delivery evicts the LRU entry
   6 a block larger than a slot is bypassed
   7 bad blocks never enter: a damaged header, a raw image one byte short, a flipped chunk byte under verify, a cut LZ4 and a cut zstd payload
   8 verify and trust: what a verify-off session inserted is a miss for a verify-on session; a flipped byte cached verify-off is served to
     verify-off sessions only
   9 refusals leave everything usable
  10 a StoreIndex that lists a cached block hash with other chunk sizes or another raw size gets a miss, not wrong bytes

In every test the output buffer is filled with 0xA5 first and compared WHOLE with what is expected.  Every comparison is equality."""
import errno

import numpy as np
import pytest
import torch

from longtail_amd.lib import BlockCache, Context, LongtailHipError, Restore
from tests.block_cache_util import CacheModel, table_digest
from tests.restore_util import BLK2, BLK3, MEOW, build_store_index, build_version_index, parse_store_index, raw_image
from tests.restore_windows_util import (FILL, LENGTHS, SWEEP_ASSETS, SWEEP_BLOCKS, expected_windows_output, model_occurrences, place, sweep_chunks,
                                        sweep_files, sweep_windows)
from tests.test_gpu_ingest_by_tag import CONFIGS, LZ4
from tests.test_gpu_ingest_stream import _sessions
from tests.test_gpu_restore import _open, deliver, expected_output, files_of, keep, written
from tests.test_gpu_restore_windows import chunk_span, same, sweep

pytestmark = pytest.mark.gpu
RAW = [sum(LENGTHS[c] for c in cs) for cs in SWEEP_BLOCKS]  # 32, 50, 4352


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    yield
    while _open:  # (last opened first: the sessions before their cache)
        _open.pop().close()
    while _sessions:
        _sessions.pop().close()


def refused(code, fn):
    with pytest.raises(LongtailHipError) as e:
        fn()
    assert e.value.code == code, (e.value.code, code)


def serve(gpu, vi, si, images, cache, out_bytes, verify=True, windows=None, offsets=None, batches=1, from_cache_at=0, finish=True):
    """A session with `cache` attached (None: without), fed its needed blocks in `batches` calls from `images` (by block hash);
    from_cache comes in front of call number from_cache_at (>= batches: behind the last) -> (finish's code, result, output, session)."""
    rs = keep(Restore(gpu, vi, si, offsets, out_bytes, verify=verify, windows=windows))
    if cache is not None:
        rs.set_cache(cache)
    out = torch.full((max(out_bytes, 1),), FILL, dtype=torch.uint8, device="cuda")
    needed = rs.needed_blocks()
    for k in range(batches):
        if cache is not None and from_cache_at == k:
            rs.from_cache(out)
        mine = needed[k::batches]
        if len(mine):
            deliver(rs, mine, [images[int(h)] for h in mine], out)
    if cache is not None and from_cache_at >= batches:
        rs.from_cache(out)
    if not finish:
        return None, None, out, rs
    code, res = rs.finish()
    return code, res, out.cpu().numpy()[:out_bytes], rs


def block_windows(blocks):
    """Windows of the sweep that need exactly these blocks: the first chunk of each, where it lies in asset 0 (chunk c is its c-th)."""
    return place([(0, *chunk_span(0, SWEEP_BLOCKS[b][0])) for b in blocks])


def sweep_metas(s):
    return [(len(cs), RAW[b], table_digest(s["hashes"][cs], [LENGTHS[c] for c in cs])) for b, cs in enumerate(SWEEP_BLOCKS)]


# ---- 1. a second session needs nothing ----


@pytest.mark.parametrize("verify", [True, False])
def test_a_second_session_needs_nothing(gpu, oracle, verify):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    occ, _ = model_occurrences(s["vi"], windows)
    want = expected_windows_output(s["files"], windows, out_bytes)
    cache = keep(BlockCache(gpu, 3, 4352))
    assert cache.stats() == dict(slots=3, slot_bytes=4352, resident=0, pinned=0, reserved=0, hits=0, inserted=0, evicted=0, bypassed=0, dropped=0)
    code, res_a, out_a, a = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, verify=verify, windows=windows)
    assert code == 0 and a.cache_stats() == (0, 0, 3, 0, 0, 0)
    same(out_a, want)
    assert cache.contains(BLK3, s["block_hashes"]).tolist() == [1, 1, 1] and cache.contains(BLK2, s["block_hashes"]).tolist() == [0, 0, 0]
    b = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, verify=verify, windows=windows))
    b.set_cache(cache)
    assert len(b.needed_blocks()) == 0 and b.scratch_bound(s["block_hashes"]) == 0
    assert cache.stats()["pinned"] == 3
    out = torch.full((out_bytes,), FILL, dtype=torch.uint8, device="cuda")
    code, _ = b.finish()
    assert code == errno.ENOENT, "cache-fed blocks exist and from_cache has not been called"
    b.from_cache(out)
    code, res_b = b.finish()
    assert code == 0 and res_b.blocks_needed == 0 and res_b.blocks_delivered == 0 and res_b.decoded_bytes == 0
    same(out.cpu().numpy(), out_a)
    assert b.cache_stats() == (3, sum(RAW), 0, 0, 0, len(occ))
    assert (res_b.occurrences, res_b.occurrences_written, res_b.bytes_written) == (res_a.occurrences, res_a.occurrences_written, res_a.bytes_written)
    st = cache.stats()
    assert (st["resident"], st["pinned"], st["reserved"], st["hits"], st["inserted"], st["evicted"]) == (3, 0, 0, 3, 3, 0)
    cache.clear()
    assert cache.stats()["resident"] == 0 and cache.contains(BLK3, s["block_hashes"]).tolist() == [0, 0, 0]


# ---- 2. tagged stores ----

# (the fixture's 'meow' run passes no asset tags, so it writes no by-tag store: every other pair of codec and hash type)
TAGGED = [(codec, h) for codec in ("lz4", "zstd", "by-tag") for h in (BLK3, BLK2)] + [("lz4", MEOW), ("zstd", MEOW)]


def store_of(w):
    si = parse_store_index(w["si"])
    images = {int(h): i for h, i in zip(si["block_hashes"], w["images"])}
    raws = [int(si["chunk_sizes"][int(o) : int(o) + int(n)].sum()) for o, n in zip(si["block_offsets"], si["block_counts"])]
    return si, images, raws


@pytest.mark.parametrize("codec,hash_id", TAGGED)
def test_tagged_stores_are_served_from_the_cache(gpu, oracle, ref, codec, hash_id):
    w = written(gpu, oracle, ref, codec, CONFIGS[0], hash_id)
    files = files_of(w["tree"])
    si, images, raws = store_of(w)
    assert (si["block_tags"] != 0).any()
    offsets, total = Restore.layout(w["vi"], 64)
    want = expected_output(files, offsets, total)
    cache = keep(BlockCache(gpu, len(raws), max(raws)))
    code, res, out, a = serve(gpu, w["vi"], w["si"], images, cache, total, offsets=offsets)
    assert code == 0 and a.cache_stats() == (0, 0, len(raws), 0, 0, 0) and res.decoded_bytes > 0
    same(out, want)
    assert cache.contains(hash_id, si["block_hashes"]).all()
    # ---- 64 random windows, wholly from the cache ----
    rng = np.random.default_rng(64)
    real = [a for a, f in enumerate(files) if len(f)]
    spans = []
    for _ in range(64):
        a = int(rng.choice(real))
        off = int(rng.integers(0, len(files[a])))
        spans.append((a, off, int(rng.integers(1, len(files[a]) - off + 1))))
    windows, out_bytes = place(spans)
    code, res, out, b = serve(gpu, w["vi"], w["si"], images, cache, out_bytes, windows=windows)
    assert code == 0 and len(b.needed_blocks()) == 0 and res.decoded_bytes == 0 and res.blocks_delivered == 0
    same(out, expected_windows_output(files, windows, out_bytes))
    assert res.bytes_written == sum(n for _, _, n, _ in windows)
    # ---- and the full restore from the cache alone ----
    code, res, out, c = serve(gpu, w["vi"], w["si"], images, cache, total, offsets=offsets)
    assert code == 0 and len(c.needed_blocks()) == 0 and res.decoded_bytes == 0 and res.bytes_written == sum(len(f) for f in files)
    same(out, want)
    assert c.cache_stats()[:2] == (len(raws), sum(raws))


# ---- 3. mixed feeding ----


def half_filled(gpu, w, images, raws, offsets, total):
    """A cache that holds every second block of the store: a session that delivers only those and is closed unfinished-for-the-rest."""
    si = parse_store_index(w["si"])
    cache = keep(BlockCache(gpu, len(raws), max(raws)))
    rs = keep(Restore(gpu, w["vi"], w["si"], offsets, total, verify=True))
    rs.set_cache(cache)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    mine = si["block_hashes"][0::2]
    deliver(rs, mine, [images[int(h)] for h in mine], out)
    code, _ = rs.finish()
    assert code == errno.ENOENT and rs.cache_stats()[2] == len(mine), "the good blocks are committed by any finish"
    rs.close()
    held = cache.contains(si["hash_id"], si["block_hashes"]).tolist()
    assert held == [1 if b % 2 == 0 else 0 for b in range(len(raws))]
    return cache, held


@pytest.mark.parametrize("batches,at", [(1, 0), (1, 1), (3, 0), (3, 1), (3, 2), (3, 3)])
def test_cached_and_delivered_blocks_in_any_order(gpu, oracle, ref, batches, at):
    w = written(gpu, oracle, ref, "by-tag", CONFIGS[0])
    files = files_of(w["tree"])
    si, images, raws = store_of(w)
    assert len(raws) >= 4 and len(set(si["block_tags"].tolist())) >= 3
    offsets, total = Restore.layout(w["vi"], 64)
    cache, held = half_filled(gpu, w, images, raws, offsets, total)
    code, res, out, rs = serve(gpu, w["vi"], w["si"], images, cache, total, offsets=offsets, batches=batches, from_cache_at=at)
    assert code == 0
    same(out, expected_output(files, offsets, total))
    fed = [b for b, h in enumerate(held) if h]
    assert rs.cache_stats()[:5] == (len(fed), sum(raws[b] for b in fed), len(raws) - len(fed), 0, 0)
    assert res.blocks_needed == res.blocks_delivered == len(raws) - len(fed) and res.bytes_written == sum(len(f) for f in files)
    assert res.decoded_bytes == sum(raws[b] for b in range(len(raws)) if not held[b] and si["block_tags"][b])
    assert cache.contains(si["hash_id"], si["block_hashes"]).all()


def based(oracle):
    """The sweep's version as the target of an update: the base holds chunks 0 and 3 in one asset, so every block is still needed."""
    s = sweep(oracle)
    base_files = [np.concatenate([sweep_chunks()[0], sweep_chunks()[3]])]
    base_vi = build_version_index(BLK3, 32768, ["b"], [[0, 1]], s["hashes"][[0, 3]], [LENGTHS[0], LENGTHS[3]])
    return s, base_vi, base_files


@pytest.mark.parametrize("verify", [True, False])
def test_mixed_feeding_on_a_session_from_a_base(gpu, oracle, verify):
    s, base_vi, base_files = based(oracle)
    sizes = [len(f) for f in s["files"]]
    offsets = np.array([5, 5 + sizes[0] + 3, 5 + sizes[0] + sizes[1] + 9], np.uint64)
    total = int(offsets[2]) + sizes[2] + 7
    cache = keep(BlockCache(gpu, 3, 4352))
    a = keep(Restore(gpu, s["vi"], s["si"], offsets, total, verify=verify))
    a.set_cache(cache)
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    deliver(a, s["block_hashes"][[0, 2]], [s["images"][int(h)] for h in s["block_hashes"][[0, 2]]], out)
    assert a.finish()[0] == errno.ENOENT
    a.close()
    base = torch.from_numpy(np.concatenate([np.full(11, 0x77, np.uint8), base_files[0]])).cuda()
    rs = keep(Restore(gpu, s["vi"], s["si"], offsets, total, verify=verify, base=(base_vi, np.array([11], np.uint64), 11 + len(base_files[0]))))
    rs.set_cache(cache)
    assert rs.needed_blocks().tolist() == [int(s["block_hashes"][1])]
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    rs.from_cache(out)
    rs.carry(base, out)
    deliver(rs, s["block_hashes"][[1]], [s["images"][int(s["block_hashes"][1])]], out)
    code, res = rs.finish()
    assert code == 0 and res.base_occurrences > 0 and res.bytes_written == sum(sizes) and res.blocks_needed == 1
    same(out.cpu().numpy(), expected_output(s["files"], offsets, total))
    assert rs.cache_stats()[:5] == (2, RAW[0] + RAW[2], 1, 0, 0)


def test_mixed_feeding_on_an_update_in_place_and_its_order(gpu, oracle):
    s, base_vi, base_files = based(oracle)
    sizes = [len(f) for f in s["files"]]
    n_base = len(base_files[0])
    offsets = np.array([64, 64 + sizes[0] + 3, 64 + sizes[0] + sizes[1] + 9], np.uint64)
    total = int(offsets[2]) + sizes[2] + 7
    host = np.random.default_rng(5).integers(0, 256, total).astype(np.uint8)
    host[3 : 3 + n_base] = base_files[0]
    base = (base_vi, np.array([3], np.uint64), 3 + n_base)
    cache = keep(BlockCache(gpu, 3, 4352))
    fill = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    a = keep(Restore(gpu, s["vi"], s["si"], offsets, total, verify=True))
    a.set_cache(cache)
    deliver(a, s["block_hashes"][[0, 2]], [s["images"][int(h)] for h in s["block_hashes"][[0, 2]]], fill)
    assert a.finish()[0] == errno.ENOENT
    a.close()
    # ---- from_cache counts as a blocks call: the carry in place comes first ----
    buf = torch.from_numpy(host).cuda()
    x = keep(Restore(gpu, s["vi"], s["si"], offsets, total, verify=True, base=base))
    x.set_cache(cache)
    scratch = torch.zeros(x.in_place_scratch_bound() + 16, dtype=torch.uint8, device="cuda")
    x.from_cache(buf)
    refused(errno.EINVAL, lambda: x.carry_in_place(buf, scratch))
    x.close()
    # ---- carry in place, then from_cache: into that buffer only ----
    buf = torch.from_numpy(host).cuda()
    rs = keep(Restore(gpu, s["vi"], s["si"], offsets, total, verify=True, base=base))
    rs.set_cache(cache)
    assert rs.needed_blocks().tolist() == [int(s["block_hashes"][1])] and rs.in_place_stats()[2] > 0
    rs.carry_in_place(buf, scratch)
    refused(errno.EINVAL, lambda: rs.from_cache(fill))
    deliver(rs, s["block_hashes"][[1]], [s["images"][int(s["block_hashes"][1])]], buf)
    rs.from_cache(buf)
    refused(errno.EEXIST, lambda: rs.from_cache(buf))
    code, res = rs.finish()
    assert code == 0 and res.bytes_written == sum(sizes)
    want = host.copy()
    for f, o in zip(s["files"], offsets.tolist()):
        want[o : o + len(f)] = f
    same(buf.cpu().numpy(), want)
    assert rs.cache_stats()[:5] == (2, RAW[0] + RAW[2], 1, 0, 0) and cache.stats()["pinned"] == 0


# ---- 4. LRU against the model ----

SCRIPT = [([0], True), ([1], True), ([0], True), ([2], True), ([1, 2], True), ([0, 1], False), ([0, 1, 2], True), ([2], False), ([0], True),
          ([1], False), ([0, 1, 2], False), ([1], True)]


def model_session(model, s, blocks, verify):
    """What a finished session that needs `blocks` (StoreIndex order) does to the cache -> (cache-fed, inserted, bypassed)."""
    metas = sweep_metas(s)
    key = lambda b: (BLK3, int(s["block_hashes"][b]))
    pinned = [(b, model.attach(key(b), metas[b], verify)) for b in blocks]
    reserved = [(b, model.reserve(key(b), metas[b])) for b, slot in pinned if slot < 0]
    inserted = sum(model.commit(slot, verify) for _, slot in reserved if slot >= 0)
    for _, slot in pinned:
        if slot >= 0:
            model.unpin(slot)
    return sum(slot >= 0 for _, slot in pinned), inserted, sum(slot < 0 for _, slot in reserved)


def test_replacement_is_the_models_lru(gpu, oracle):
    s = sweep(oracle)
    cache = keep(BlockCache(gpu, 2, 4352))
    model = CacheModel(2, 4352)
    evictions = 0
    for blocks, verify in SCRIPT:
        windows, out_bytes = block_windows(blocks)
        code, res, out, rs = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, verify=verify, windows=windows)
        assert code == 0
        same(out, expected_windows_output(s["files"], windows, out_bytes))
        fed, inserted, bypassed = model_session(model, s, blocks, verify)
        assert rs.cache_stats()[0] == fed and rs.cache_stats()[2:5] == (inserted, bypassed, 0), (blocks, verify)
        held = [int((BLK3, int(h)) in model.resident()) for h in s["block_hashes"]]
        assert cache.contains(BLK3, s["block_hashes"]).tolist() == held, (blocks, verify)
        st = cache.stats()
        assert (st["hits"], st["inserted"], st["evicted"], st["bypassed"]) == (model.hits, model.inserted, model.evicted, model.bypassed)
        rs.close()
    assert model.evicted >= 4 and model.bypassed >= 1 and model.hits >= 3, "the script replaces, bypasses and hits"


# ---- 5. pins ----


def test_pinned_entries_are_not_replaced(gpu, oracle):
    s = sweep(oracle)
    cache = keep(BlockCache(gpu, 2, 4352))
    hashes = s["block_hashes"]
    w01, n01 = block_windows([0, 1])
    assert serve(gpu, s["vi"], s["si"], s["images"], cache, n01, windows=w01)[0] == 0
    holders = []
    for b in (0, 1):
        w, n = block_windows([b])
        holders.append((serve(gpu, s["vi"], s["si"], s["images"], cache, n, windows=w, finish=False), w, n))
    assert cache.stats()["pinned"] == 2
    refused(errno.EBUSY, cache.clear)
    w2, n2 = block_windows([2])
    code, res, out, t = serve(gpu, s["vi"], s["si"], s["images"], cache, n2, windows=w2)
    assert code == 0 and t.cache_stats() == (0, 0, 0, 1, 0, 0)
    same(out, expected_windows_output(s["files"], w2, n2))
    assert cache.contains(BLK3, hashes).tolist() == [1, 1, 0]
    for (_, _, out, rs), w, n in holders:
        assert rs.finish()[0] == 0
        same(out.cpu().numpy()[:n], expected_windows_output(s["files"], w, n))
    assert cache.stats()["pinned"] == 0
    # block 0 was used before block 1 (both by their holders' set_cache): it goes
    code, res, out, u = serve(gpu, s["vi"], s["si"], s["images"], cache, n2, windows=w2)
    assert code == 0 and u.cache_stats() == (0, 0, 1, 0, 0, 0)
    assert cache.contains(BLK3, hashes).tolist() == [0, 1, 1] and cache.stats()["evicted"] == 1


# ---- 6. too large ----


def test_a_block_larger_than_a_slot_is_bypassed(gpu, oracle):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    cache = keep(BlockCache(gpu, 3, 50))
    assert cache.stats()["slot_bytes"] == 64
    code, res, out, a = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, windows=windows)
    assert code == 0 and a.cache_stats() == (0, 0, 2, 1, 0, 0)
    want = expected_windows_output(s["files"], windows, out_bytes)
    same(out, want)
    assert cache.contains(BLK3, s["block_hashes"]).tolist() == [1, 1, 0]
    b = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, windows=windows))
    b.set_cache(cache)
    assert b.needed_blocks().tolist() == [int(s["block_hashes"][2])]
    b.close()
    code, res, out, b = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, windows=windows, from_cache_at=1)
    assert code == 0 and b.cache_stats()[:5] == (2, RAW[0] + RAW[1], 0, 1, 0)
    same(out, want)


# ---- 7. bad blocks never enter ----


def check_bad_block(gpu, vi, si, images, bad_hash, bad_image, hash_id, verify, want, out_bytes, slot_bytes, offsets=None, windows=None):
    hashes = parse_store_index(si)["block_hashes"]
    cache = keep(BlockCache(gpu, len(hashes), slot_bytes))
    damaged = dict(images)
    damaged[int(bad_hash)] = bad_image
    code, res, out, a = serve(gpu, vi, si, damaged, cache, out_bytes, verify=verify, offsets=offsets, windows=windows)
    assert code == errno.EBADF and res.blocks_bad == 1
    assert a.cache_stats() == (0, 0, len(hashes) - 1, 0, 1, 0) and cache.stats()["dropped"] == 1 and cache.stats()["reserved"] == 0
    assert cache.contains(hash_id, hashes).tolist() == [int(int(h) != int(bad_hash)) for h in hashes]
    a.close()
    b = keep(Restore(gpu, vi, si, offsets, out_bytes, verify=verify, windows=windows))
    b.set_cache(cache)
    assert b.needed_blocks().tolist() == [int(bad_hash)]
    out = torch.full((out_bytes,), FILL, dtype=torch.uint8, device="cuda")
    deliver(b, np.array([bad_hash], np.uint64), [images[int(bad_hash)]], out)
    b.from_cache(out)
    assert b.finish()[0] == 0
    same(out.cpu().numpy(), want)
    assert cache.contains(hash_id, hashes).all()


@pytest.mark.parametrize("case", ["header", "one byte short", "chunk byte"])
def test_a_bad_raw_block_never_enters(gpu, oracle, case):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    bad = int(s["block_hashes"][2])
    image = s["images"][bad].copy()
    if case == "header":
        image[20 + 3] ^= 0x10  # a bit of the first chunk hash
    elif case == "one byte short":
        image = image[:-1].copy()
    else:
        image[20 + 12 * len(SWEEP_BLOCKS[2]) + 300] ^= 0x01
    check_bad_block(gpu, s["vi"], s["si"], s["images"], bad, image, BLK3, True, expected_windows_output(s["files"], windows, out_bytes), out_bytes,
                    4352, windows=windows)


@pytest.mark.parametrize("codec", ["lz4", "zstd"])
def test_a_block_with_a_cut_payload_never_enters(gpu, oracle, ref, codec):
    """Half of the payload is cut off and the header's compressed size follows: a right header over a payload that the reference's
    decoder rejects as well."""
    w = written(gpu, oracle, ref, codec, CONFIGS[0])
    files = files_of(w["tree"])
    si, images, raws = store_of(w)
    b = int(np.flatnonzero(si["block_tags"] != 0)[0])
    bad = int(si["block_hashes"][b])
    hdr = 20 + 12 * int(si["block_counts"][b]) + 8
    good = images[bad]
    keep_bytes = (len(good) - hdr) // 2
    assert keep_bytes > 8
    image = good[: hdr + keep_bytes].copy()
    image[hdr - 4 : hdr] = np.array([keep_bytes], np.uint32).view(np.uint8)
    payload = np.ascontiguousarray(image[hdr:])
    if codec == "lz4":
        assert oracle.lz4_decompress(payload, raws[b])[0] != raws[b]
    else:
        assert ref.decompress(1, payload, raws[b])[0] != 0
    offsets, total = Restore.layout(w["vi"], 64)
    check_bad_block(gpu, w["vi"], w["si"], images, bad, image, si["hash_id"], False, expected_output(files, offsets, total), total, max(raws),
                    offsets=offsets)


# ---- 8. verify and trust ----


def test_a_verifying_session_reads_only_what_a_verifying_session_wrote(gpu, oracle):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    want = expected_windows_output(s["files"], windows, out_bytes)
    cache = keep(BlockCache(gpu, 3, 4352))
    assert serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, verify=False, windows=windows)[0] == 0
    b = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, verify=True, windows=windows))
    b.set_cache(cache)
    assert (b.needed_blocks() == s["block_hashes"]).all(), "unverified entries are misses for a verify session"
    b.close()
    code, res, out, b = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, verify=True, windows=windows)
    assert code == 0 and b.cache_stats() == (0, 0, 3, 0, 0, 0) and cache.stats()["evicted"] == 3, "the slots are reused in place"
    same(out, want)
    for verify in (True, False):
        code, res, out, c = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, verify=verify, windows=windows)
        assert code == 0 and len(c.needed_blocks()) == 0 and c.cache_stats()[0] == 3
        same(out, want)


def test_what_verify_off_trusts_is_served_to_verify_off_sessions_only(gpu, oracle):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    bad = int(s["block_hashes"][2])
    flipped = dict(s["images"])
    flipped[bad] = s["images"][bad].copy()
    flipped[bad][20 + 12 * len(SWEEP_BLOCKS[2]) + 300] ^= 0x01  # byte 300 of the block: byte 45 of chunk 6
    chunks = sweep_chunks()
    chunks[6] = chunks[6].copy()
    chunks[6][300 - LENGTHS[5]] ^= 0x01
    want_flipped = expected_windows_output(sweep_files(chunks), windows, out_bytes)
    want = expected_windows_output(s["files"], windows, out_bytes)
    assert (want_flipped != want).any()
    cache = keep(BlockCache(gpu, 3, 4352))
    code, res, out, a = serve(gpu, s["vi"], s["si"], flipped, cache, out_bytes, verify=False, windows=windows)
    assert code == 0 and a.cache_stats()[2] == 3
    same(out, want_flipped)
    code, res, out, b = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, verify=False, windows=windows)
    assert code == 0 and len(b.needed_blocks()) == 0
    same(out, want_flipped)  # the documented trust of verify-off
    code, res, out, c = serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, verify=True, windows=windows)
    assert code == 0 and (c.needed_blocks() == s["block_hashes"]).all()
    same(out, want)


# ---- 9. refusals ----


def test_refusals_leave_everything_usable(gpu, gpu_abl, oracle):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    want = expected_windows_output(s["files"], windows, out_bytes)
    dll = gpu.lib.dll
    for slots, size in ((0, 64), (4, 0)):
        refused(errno.EINVAL, lambda: BlockCache(gpu, slots, size))
    cache, other = keep(BlockCache(gpu, 3, 4352)), keep(BlockCache(gpu, 1, 64))
    foreign = keep(BlockCache(keep(Context(0)), 1, 64))
    out = torch.full((out_bytes,), FILL, dtype=torch.uint8, device="cuda")
    rs = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, windows=windows))
    refused(errno.EINVAL, lambda: rs.from_cache(out))  # without a cache
    refused(errno.EINVAL, lambda: rs.set_cache(None))
    assert dll.lthip_restore_set_cache(None, cache.h) == errno.EINVAL
    refused(errno.EINVAL, lambda: rs.set_cache(foreign))  # another context's
    rs.set_cache(cache)
    refused(errno.EEXIST, lambda: rs.set_cache(cache))
    refused(errno.EEXIST, lambda: rs.set_cache(other))
    deliver(rs, s["block_hashes"], [s["images"][int(h)] for h in s["block_hashes"]], out)
    rs.from_cache(out)  # (nothing is cache-fed: it queues nothing)
    refused(errno.EEXIST, lambda: rs.from_cache(out))
    assert rs.finish()[0] == 0
    same(out.cpu().numpy(), want)
    late = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, windows=windows))
    out2 = torch.full((out_bytes,), FILL, dtype=torch.uint8, device="cuda")
    deliver(late, s["block_hashes"][[1]], [s["images"][int(s["block_hashes"][1])]], out2)
    refused(errno.EINVAL, lambda: late.set_cache(cache))  # after a blocks call
    deliver(late, s["block_hashes"][[0, 2]], [s["images"][int(h)] for h in s["block_hashes"][[0, 2]]], out2)
    assert late.finish()[0] == 0 and late.cache_stats() == (0, 0, 0, 0, 0, 0)
    same(out2.cpu().numpy(), want)
    # ---- clear while pinned ----
    pin = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, windows=windows))
    pin.set_cache(cache)
    refused(errno.EBUSY, cache.clear)
    assert cache.contains(BLK3, s["block_hashes"]).tolist() == [1, 1, 1]
    out3 = torch.full((out_bytes,), FILL, dtype=torch.uint8, device="cuda")
    pin.from_cache(out3)
    assert pin.finish()[0] == 0
    same(out3.cpu().numpy(), want)
    cache.clear()
    # ---- no memory for the arena: nothing stays allocated, the context works ----
    abl = gpu_abl.lib.dll
    try:
        assert abl.lthip_debug_fail_alloc(0, 1) == 0
        refused(errno.ENOMEM, lambda: BlockCache(gpu_abl, 3, 4352))
    finally:
        abl.lthip_debug_fail_alloc(-1, 0)
    again = keep(BlockCache(gpu_abl, 3, 4352))
    code, res, got, _ = serve(gpu_abl, s["vi"], s["si"], s["images"], again, out_bytes, windows=windows)
    assert code == 0
    same(got, want)
    code, res, got, rs = serve(gpu_abl, s["vi"], s["si"], s["images"], again, out_bytes, windows=windows)
    assert code == 0 and rs.cache_stats()[0] == 3
    same(got, want)


# ---- 10. a different StoreIndex ----


@pytest.mark.parametrize("sizes", [(18, 32), (17, 34)], ids=["other chunk sizes", "another raw size"])
def test_a_store_index_that_lists_the_block_differently_gets_a_miss(gpu, oracle, sizes):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    cache = keep(BlockCache(gpu, 3, 4352))
    assert serve(gpu, s["vi"], s["si"], s["images"], cache, out_bytes, windows=windows)[0] == 0
    # the same block hashes; block 1's two chunks are other chunks of other sizes
    lengths = LENGTHS[:3] + list(sizes) + LENGTHS[5:]
    rng = np.random.default_rng(77)
    chunks = sweep_chunks()
    chunks[3], chunks[4] = (rng.integers(0, 256, n).astype(np.uint8) for n in sizes)
    content = np.concatenate(chunks)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    hashes = oracle.blake3_many(content, starts, lengths)
    assert (hashes[[0, 1, 2, 5, 6]] == s["hashes"][[0, 1, 2, 5, 6]]).all()
    vi = build_version_index(BLK3, 32768, [f"s{a}" for a in range(len(SWEEP_ASSETS))], SWEEP_ASSETS, hashes, lengths)
    si = build_store_index(BLK3, [(int(h), 0, cs) for h, cs in zip(s["block_hashes"], SWEEP_BLOCKS)], hashes, lengths)
    lens = np.array(lengths, np.uint32)
    images = dict(s["images"])
    h1 = int(s["block_hashes"][1])
    images[h1] = raw_image(h1, BLK3, hashes[SWEEP_BLOCKS[1]], lens[SWEEP_BLOCKS[1]], np.concatenate([chunks[c] for c in SWEEP_BLOCKS[1]]))
    files = [np.concatenate([chunks[c] for c in cs]) for cs in SWEEP_ASSETS]
    spans = [(a, 0, len(f)) for a, f in enumerate(files)] + [(2, 1, len(files[2]) - 2)]
    mine, n = place(spans)
    rs = keep(Restore(gpu, vi, si, None, n, windows=mine))
    rs.set_cache(cache)
    assert rs.needed_blocks().tolist() == [h1], "blocks 0 and 2 are listed as they were: hits; block 1 is a miss"
    rs.close()
    code, res, out, rs = serve(gpu, vi, si, images, cache, n, windows=mine)
    assert code == 0 and rs.cache_stats()[:5] == (2, RAW[0] + RAW[2], 1, 0, 0)
    same(out, expected_windows_output(files, mine, n))
    assert cache.stats()["evicted"] == 1, "the entry that did not match gave its slot"
    # ... and the first StoreIndex now misses block 1 in turn
    back = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, windows=windows))
    back.set_cache(cache)
    assert back.needed_blocks().tolist() == [h1]
