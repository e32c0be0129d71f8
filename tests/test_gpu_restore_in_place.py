"""-m gpu: updating a resident version IN PLACE (lthip_restore_layout_in_place, lthip_restore_carry_in_place, lthip_restore_in_place_stats,
lthip_restore_in_place_scratch_bound; include/longtail_hip.h, "updating a resident version in place") -- version N lies restored in a
buffer, and version N + 1 is made in that same buffer: what both share stays or moves through a scratch, the rest comes out of blocks.

  1. a hazard sweep on versions built by hand, verify off and on: an asset kept; assets shifted up and down by 1, 15, 16, 17 and 4097
     bytes, each less than its length; a 300 KiB asset shifted by 100 and by 40 000 bytes; two assets of different sizes that swap places;
     a chunk inserted in front of an asset that stays where it was; a store-fed chunk on the source of a chunk moved later in the list;
     moved chunks whose destinations are the sources of other moved chunks, in both list orders; every source and destination residue
     mod 16; chunks that start and end at the last byte of the buffer; one base chunk feeding a kept and moved occurrences
  2. version A -> version B of tests/test_gpu_ingest_store.py at the offsets of lthip_restore_layout_in_place, 'blk3', 'blk2' and 'meow'
  3. a damaged base chunk, kept or moved, with and without verify
  4. refusals and the order of the calls; a session in which everything is kept
  5. scratch of exactly lthip_restore_in_place_scratch_bound bytes at the end of its allocation

The buffer is filled with a pattern first, and the WHOLE buffer is compared with what a numpy model makes of a snapshot taken before the
call: a base-fed occurrence is the snapshot's bytes at the chunk's first place in the base, a store-fed one the chunk, everything else
what it was.  Every comparison is equality."""
import errno

import numpy as np
import pytest
import torch

from longtail_amd.lib import LongtailHipError, Restore, Store, restore_layout_in_place
from tests import test_gpu_ingest_store as store_tests
from tests.restore_util import BLK2, BLK3, MEOW, build_store_index, parse_store_index, raw_image
from tests.test_gpu_ingest_store import STORE_CONFIGS, next_version, tag_of
from tests.test_gpu_ingest_stream import _sessions, chunk_jobs, index_buffers, open_stream, slices_of, stream_tree, tree_of
from tests.test_gpu_restore import FILL, deliver, expected_output, files_of, occurrences
from tests.test_gpu_restore_update import device_hashes, first_places, refused, version_of, versions

pytestmark = pytest.mark.gpu

_open, _scenes, _hashed = [], {}, {}
GUARD = 4097  # bytes in front of the scratch: an odd number, so that the scratch starts on no 16-byte boundary


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    yield
    for held in (_open, store_tests._open, _sessions):
        while held:
            held.pop().close()


def keep(obj):
    _open.append(obj)
    return obj


def model(snapshot, base_vi, base_offsets, vi, offsets, fresh, bad=()):
    """-> (the buffer after the update, in_place_stats, the base-fed occurrences).  fresh: the target restored from scratch at `offsets`;
    bad: hashes of base chunks verify rejects (their moved occurrences keep what the buffer held)."""
    places = first_places(base_vi, base_offsets)
    want, stats, fed = snapshot.copy(), [0, 0, 0, 0], []
    for h, at, n in occurrences(vi, offsets):
        if h in places and places[h][1] == n:
            src = places[h][0]
            fed.append((h, at, n, src))
            stats[0 if src == at else 2] += 1
            stats[1 if src == at else 3] += n
            if h not in bad:
                want[at : at + n] = snapshot[src : src + n]
        else:
            want[at : at + n] = fresh[at : at + n]
    return want, tuple(stats), fed


def pattern(n, seed=99):
    return np.random.default_rng(seed).integers(0, 256, max(n, 1)).astype(np.uint8)


def resident(c, damage=()):
    """The buffer with the base in it, on the host: a pattern, the base's assets at their offsets, `damage`: offsets of bytes to flip."""
    host = pattern(max(c["base_bytes"], c["out_bytes"]))
    for off, data in zip(c["base_offsets"].tolist(), c["base_files"]):
        if off != Restore.SKIP and len(data):
            host[off : off + len(data)] = data
    for at in damage:
        host[at] ^= 0x40
    return host


def update_in_place(gpu, c, host, verify, calls=2):
    """Carry in place, then the needed blocks in `calls` calls -> (finish's code, the result, the buffer, the session, the scratch's guard)"""
    index_of = {int(h): b for b, h in enumerate(parse_store_index(c["si"])["block_hashes"])}
    rs = keep(Restore(gpu, c["vi"], c["si"], c["offsets"], c["out_bytes"], verify=verify, base=(c["base_vi"], c["base_offsets"], c["base_bytes"])))
    buf = torch.from_numpy(host).cuda()
    bound = rs.in_place_scratch_bound()
    alloc = torch.full((GUARD + bound,), 0x3C, dtype=torch.uint8, device="cuda")
    rs.carry_in_place(buf, alloc[GUARD:] if bound else None)
    needed = [int(h) for h in rs.needed_blocks()]
    cut = len(needed) // 2 if calls == 2 else len(needed)
    for part in (needed[:cut], needed[cut:]):
        if part:
            deliver(rs, np.array(part, np.uint64), [c["images"][index_of[h]] for h in part], buf)
    code, res = rs.finish()
    return code, res, buf.cpu().numpy(), rs, alloc[:GUARD].cpu().numpy()


def same(got, want):
    assert got.shape == want.shape and (got == want).all(), int(np.flatnonzero(got != want)[0])


# ---- 1. the hazard sweep ----


class Scene:
    def __init__(self, seed):
        self.rng, self.pool, self.base, self.target, self.at = np.random.default_rng(seed), [], [], [], 7

    def new(self, n):
        self.pool.append(self.rng.integers(0, 256, int(n)).astype(np.uint8))
        return len(self.pool) - 1

    def size(self, cs):
        return sum(len(self.pool[c]) for c in cs)

    def region(self, n):
        self.at += n
        return self.at - n

    def case(self, gpu, hash_id, store_chunks, base_bytes, out_bytes, skip=()):
        """store_chunks: the chunks of each block of the store (raw blocks)"""
        hashes = device_hashes(gpu, hash_id, self.pool)
        assert len(set(hashes.tolist())) == len(self.pool)
        sizes = [len(c) for c in self.pool]
        files = lambda assets: [np.concatenate([self.pool[c] for c in cs]) if cs else np.zeros(0, np.uint8) for _, _, cs in assets]
        blocks = [(0xB10C0 + b, 0, cs) for b, cs in enumerate(store_chunks)]
        images = [raw_image(bh, hash_id, [hashes[c] for c in cs], [sizes[c] for c in cs], np.concatenate([self.pool[c] for c in cs]))
                  for bh, _, cs in blocks]
        return dict(vi=version_of(hash_id, [a[0] for a in self.target], [a[2] for a in self.target], hashes, sizes),
                    base_vi=version_of(hash_id, [a[0] for a in self.base], [a[2] for a in self.base], hashes, sizes),
                    offsets=np.array([a[1] for a in self.target], np.uint64),
                    base_offsets=np.array([Restore.SKIP if a[0] in skip else a[1] for a in self.base], np.uint64),
                    files=files(self.target), base_files=files(self.base), si=build_store_index(hash_id, blocks, hashes, sizes), images=images,
                    base_bytes=base_bytes, out_bytes=out_bytes, hashes=hashes, blocks=[0xB10C0 + b for b in range(len(blocks))])


def small_scene(gpu, hash_id=BLK3):
    """Everything of the sweep but the 300 KiB assets; -> the case and the chunk ids the other tests aim at"""
    if ("small", hash_id) in _scenes:
        return _scenes[("small", hash_id)]
    s = Scene(31)
    # an asset kept; its first chunk feeds two more occurrences elsewhere (its place in the base is the first one: here)
    k = [s.new(n) for n in (1200, 900, 33, 2000)]
    o = s.region(s.size(k) + 5)
    s.base.append(("kept", o, k)), s.target.append(("kept", o, k))
    for name in ("again", "again2"):
        s.target.append((name, s.region(1200 + 3), [k[0]]))
    # shifted up and down by less than the length
    for shift in (1, 15, 16, 17, 4097):
        for down in (False, True):
            u = [s.new(n) for n in (3000, 2000, 1500)]
            o = s.region(6500 + shift + 9)
            s.base.append((f"shift{shift}{'down' if down else 'up'}", o + shift if down else o, u))
            s.target.append((s.base[-1][0], o if down else o + shift, u))
    # source residue r, destination residue (7 r + 3) mod 16
    for r in range(16):
        o = (s.region(176) + 15) // 16 * 16
        c = [s.new(40 + r)]
        s.base.append((f"res{r}", o + r, c)), s.target.append((f"res{r}", o + 80 + (7 * r + 3) % 16, c))
    # two assets of different sizes swap places
    a, b = [s.new(2500), s.new(2500)], [s.new(3000)]
    o = s.region(8000 + 3)
    s.base += [("swap_a", o, a), ("swap_b", o + 5000, b)]
    s.target += [("swap_a", o + 3000, a), ("swap_b", o, b)]
    # a new chunk in front of an asset that stays: every later chunk moves up onto its successor
    x, ins = [s.new(n) for n in (1000, 1100, 900, 1000, 1200, 1000)], s.new(700)
    o = s.region(s.size(x) + 700 + 3)
    s.base.append(("grown", o, x)), s.target.append(("grown", o, [ins] + x))
    # a store-fed chunk on the source of a chunk that moves LATER in the list
    m, sn = s.new(800), s.new(800)
    o = s.region(1700)
    s.base.append(("later", o, [m]))
    s.target += [("onto", o, [sn]), ("later", o + 850, [m])]
    # a ring: p -> q's place, q -> r's place, r -> p's place (a destination that is the source of a later entry, and of an earlier one)
    p, q, r = s.new(777), s.new(777), s.new(777)
    o = s.region(2400)
    s.base += [("ring_p", o, [p]), ("ring_q", o + 800, [q]), ("ring_r", o + 1600, [r])]
    s.target += [("ring_p", o + 800, [p]), ("ring_q", o + 1600, [q]), ("ring_r", o, [r])]
    # the last bytes of the buffer: a base chunk ends there (it moves down), and a moved chunk ends there afterwards
    e = [s.new(500), s.new(300)]
    o = s.region(900 + 10 + 800)
    s.base.append(("end", o + 910, e))
    s.target += [("end", o, e), ("tail", o + 810, [k[1]])]
    c = s.case(gpu, hash_id, [[ins], [sn]], s.at, s.at)
    assert c["base_offsets"][-1] + 800 == s.at == c["offsets"][-1] + 900
    c.update(k=k, ins=ins, shifted=u)
    _scenes[("small", hash_id)] = c
    return c


def big_scene(gpu, shift, down):
    """A 300 KiB asset (ten chunks: several 32 KiB pieces per run) shifted by `shift`, and a store-fed asset behind it"""
    s = Scene(32 + shift + down)
    big, sn = [s.new(30720) for _ in range(10)], s.new(5000)
    o = s.region(307200 + shift)
    s.base.append(("big", o + shift if down else o, big))
    s.target += [("new", s.region(5000 + 1), [sn])] if down else []
    s.target.append(("big", o if down else o + shift, big))
    s.target += [] if down else [("new", s.region(5000 + 1), [sn])]
    base_bytes = s.base[0][1] + 307200
    return s.case(gpu, BLK3, [[sn]], base_bytes, s.at)


def check_sweep(gpu, c, verify):
    host = resident(c)
    fresh = expected_output(c["files"], c["offsets"], len(host))
    want, stats, fed = model(host, c["base_vi"], c["base_offsets"], c["vi"], c["offsets"], fresh)
    code, res, got, rs, guard = update_in_place(gpu, c, host, verify)
    print("in_place_stats", rs.in_place_stats(), "bound", rs.in_place_scratch_bound())
    assert code == 0
    same(got, want)
    assert rs.in_place_stats() == stats and (guard == 0x3C).all()
    assert rs.in_place_scratch_bound() <= stats[3] + 16 * stats[2] + 64
    assert (res.base_occurrences, res.base_bytes) == (stats[0] + stats[2], stats[1] + stats[3])
    total = sum(len(f) for f in c["files"])
    assert (res.occurrences_written, res.bytes_written, res.base_chunks_mismatched, res.blocks_bad) == (res.occurrences, total, 0, 0)
    # ... and the model's buffer is the target: every asset's window holds the file
    for off, data in zip(c["offsets"].tolist(), c["files"]):
        assert (want[off : off + len(data)] == data).all()
    return stats, fed


@pytest.mark.parametrize("verify", [False, True])
def test_the_hazard_sweep(gpu, verify):
    c = small_scene(gpu)
    stats, fed = check_sweep(gpu, c, verify)
    kept_window = (int(c["offsets"][0]), int(c["offsets"][0]) + len(c["files"][0]))
    in_kept = [f for f in fed if kept_window[0] <= f[1] < kept_window[1]]
    assert len(in_kept) == 4 and all(src == at for _, at, _, src in in_kept), "the kept asset: zero moved bytes"
    first = int(c["hashes"][c["k"][0]])
    assert sorted(src == at for h, at, _, src in fed if h == first) == [False, False, True], "one base chunk feeds a kept and two moved occurrences"
    assert {src % 16 for _, _, _, src in fed} == set(range(16)) == {at % 16 for _, at, _, _ in fed}
    assert {at - src for _, at, _, src in fed} >= {d * s for d in (1, 15, 16, 17, 4097) for s in (1, -1)}  # (each asset: 6500 bytes)
    assert max(at + n for _, at, n, _ in fed) == len(resident(c)) == max(src + n for _, _, n, src in fed)
    assert stats[0] == 4 and stats[2] > 50


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("shift,down", [(100, False), (100, True), (40000, False), (40000, True)])
def test_a_300_kib_asset_shifted_by_less_than_its_length(gpu, shift, down, verify):
    c = big_scene(gpu, shift, down)
    stats, _ = check_sweep(gpu, c, verify)
    assert stats == (0, 0, 10, 307200)


# ---- 2. version A -> version B ----


def run_hashed(gpu, tree, cfg, tag, store, hash_id):
    """tests/test_gpu_ingest_store.run_stream with another hash type: 'blk2' from chunk_jobs, 'meow' from meow_ranges"""
    target, codec, max_block, max_chunks = cfg
    st = open_stream(gpu, stream_tree(tree, None), target, max_block, max_chunks, codec, compression_type=tag, hash_identifier=hash_id)
    st.set_store(store)
    images, chunks_all = [], 0

    def take(arena):
        _, offs, sizes = st.images()
        host = arena.cpu().numpy()
        images.extend(host[int(o) : int(o) + int(n)].copy() for o, n in zip(offs, sizes))

    for first_job, count in slices_of("three", tree["part"].job_count):
        sl = chunk_jobs(gpu, tree, target, first_job, count, hash_id if hash_id == BLK2 else BLK3)
        if hash_id == MEOW:
            gpu.meow_ranges(sl["dev"], sl["d_off"], sl["d_len"], out=sl["d_hash"], count_bound=max(1, int(sl["d_hash"].numel())),
                            d_count=sl["d_first"][count : count + 1])
        arena = torch.zeros(max(64, st.arena_bound(sl["bytes"], sl["total"])), dtype=torch.uint8, device="cuda")
        st.slice(first_job, count, sl["dev"], sl["d_off"], sl["d_len"], sl["d_hash"], sl["d_first"], sl["total"], arena)
        take(arena)
        chunks_all += sl["total"]
    arena = torch.zeros(st.arena_bound(0, 0), dtype=torch.uint8, device="cuda")
    vi, si = index_buffers(gpu, tree, chunks_all)
    res = st.finish(arena, vi, si)
    take(arena)
    return dict(vi=bytes(vi.numpy()[: res.version_index_size]), si=bytes(si.numpy()[: res.store_index_size]), images=images)


def a_to_b(gpu, oracle, ref, cfg, hash_id):
    """dict(a: vi, b: vi / si / images of the stream session against a store that holds A, files_a, files_b, offsets_a, total_a)"""
    if hash_id == BLK3:
        v = versions(gpu, oracle, ref, cfg)
        return dict(a=v["a"]["vi"], b=v["b_missing"], files_a=v["files_a"], files_b=v["files_b"], offsets_a=v["offsets_a"], total_a=v["total_a"])
    if (cfg, hash_id) not in _hashed:
        tag = tag_of(ref, cfg[1])
        tree_a, tree_b = tree_of(oracle, ref, cfg[0]), next_version(oracle, ref, cfg[0])
        store = store_tests.keep(Store(gpu, 0))
        a = run_hashed(gpu, tree_a, cfg, tag, store, hash_id)
        store.add_index(a["si"])
        b = run_hashed(gpu, tree_b, cfg, tag, store, hash_id)
        offsets_a, total_a = Restore.layout(a["vi"], 64)
        _hashed[(cfg, hash_id)] = dict(a=a["vi"], b=b, files_a=files_of(tree_a), files_b=files_of(tree_b), offsets_a=offsets_a, total_a=total_a)
        for held in (store_tests._open, _sessions):
            while held:
                held.pop().close()
    return _hashed[(cfg, hash_id)]


def in_place_case(v):
    offsets, total, kept = restore_layout_in_place(v["a"], v["offsets_a"], v["total_a"], v["b"]["vi"], 64)
    return dict(vi=v["b"]["vi"], si=v["b"]["si"], images=v["b"]["images"], offsets=offsets, out_bytes=total, files=v["files_b"], base_vi=v["a"],
                base_offsets=v["offsets_a"], base_bytes=v["total_a"], base_files=v["files_a"]), kept


@pytest.mark.parametrize("cfg,hash_id,verify", [(STORE_CONFIGS[0], BLK3, False), (STORE_CONFIGS[0], BLK3, True), (STORE_CONFIGS[1], BLK3, True),
                                                (STORE_CONFIGS[0], BLK2, True), (STORE_CONFIGS[1], MEOW, True)])
def test_the_next_version_in_the_buffer_of_the_one_before(gpu, oracle, ref, cfg, hash_id, verify):
    v = a_to_b(gpu, oracle, ref, cfg, hash_id)
    c, kept_assets = in_place_case(v)
    with_bytes = sum(1 for f in v["files_b"] if len(f))
    assert 0 < with_bytes - kept_assets <= 3, "two files modified, one added: everything else keeps its place"
    host = resident(c)
    fresh = expected_output(c["files"], c["offsets"], len(host))
    want, stats, fed = model(host, c["base_vi"], c["base_offsets"], c["vi"], c["offsets"], fresh)
    code, res, got, rs, _ = update_in_place(gpu, c, host, verify)
    print("in_place_stats", rs.in_place_stats(), "of", sum(len(f) for f in c["files"]), "bytes; bound", rs.in_place_scratch_bound())
    assert code == 0
    same(got, want)
    for off, data in zip(c["offsets"].tolist(), c["files"]):  # byte-equal to B restored from scratch at those offsets
        assert (got[off : off + len(data)] == data).all()
    assert rs.in_place_stats() == stats and stats[1] + stats[3] == res.base_bytes and stats[0] + stats[2] == res.base_occurrences
    assert stats[1] > stats[3] > 0, "more of what the base feeds stays than moves: only the tails of the two modified files and duplicates move"
    assert res.occurrences_written == res.occurrences and res.bytes_written == sum(len(f) for f in c["files"])
    # the out-of-place session over the same pair needs the same blocks
    offsets_b, total_b = Restore.layout(c["vi"], 64)
    other = keep(Restore(gpu, c["vi"], c["si"], offsets_b, total_b, verify=verify, base=(c["base_vi"], c["base_offsets"], c["base_bytes"])))
    assert rs.needed_blocks().tolist() == other.needed_blocks().tolist() == parse_store_index(c["si"])["block_hashes"].tolist()
    assert res.blocks_needed == res.blocks_delivered > 1, "delivered in two calls"


# ---- 3. a damaged base ----


@pytest.mark.parametrize("which", ["kept", "moved"])
def test_a_damaged_base_chunk(gpu, which):
    c = small_scene(gpu)
    places = first_places(c["base_vi"], c["base_offsets"])
    # kept: the last chunk of the kept asset, which feeds nothing else; moved: the kept asset's first chunk, which feeds two moved
    # occurrences as well
    victim = int(c["hashes"][c["k"][3 if which == "kept" else 0]])
    host = resident(c, damage=[places[victim][0] + 5])
    fresh = expected_output(c["files"], c["offsets"], len(host))
    hit = [o for o in occurrences(c["vi"], c["offsets"]) if o[0] == victim]
    assert len(hit) == (1 if which == "kept" else 3)
    # ---- verify: a moved occurrence keeps what the buffer held, a kept one stays what it is ----
    want, stats, _ = model(host, c["base_vi"], c["base_offsets"], c["vi"], c["offsets"], fresh, bad={victim})
    code, res, got, rs, _ = update_in_place(gpu, c, host, True)
    assert code == errno.EBADF and (res.base_chunks_mismatched, res.blocks_bad) == (1, 0)
    same(got, want)
    for _, at, n in hit:
        assert (got[at : at + n] == host[at : at + n]).all(), "no destination of the chunk is written"
    assert rs.in_place_stats() == stats
    assert res.occurrences_written == res.occurrences - len(hit)
    assert res.bytes_written == sum(len(f) for f in c["files"]) - sum(n for _, _, n in hit)
    # ---- without verify the base is trusted: the flipped byte is carried to every occurrence ----
    want, _, _ = model(host, c["base_vi"], c["base_offsets"], c["vi"], c["offsets"], fresh)
    code, res, got, _, _ = update_in_place(gpu, c, host, False)
    assert code == 0 and res.base_chunks_mismatched == 0 and res.occurrences_written == res.occurrences
    same(got, want)
    assert np.flatnonzero(got != expected_model_of_a_good_base(c)).tolist() == sorted(at + 5 for _, at, _ in hit)


def expected_model_of_a_good_base(c):
    host = resident(c)
    return model(host, c["base_vi"], c["base_offsets"], c["vi"], c["offsets"], expected_output(c["files"], c["offsets"], len(host)))[0]


# ---- 4. refusals and order ----


def session(gpu, c, verify=True, base=True):
    return keep(Restore(gpu, c["vi"], c["si"], c["offsets"], c["out_bytes"], verify=verify,
                        base=(c["base_vi"], c["base_offsets"], c["base_bytes"]) if base else None))


def test_refusals_leave_the_session_usable(gpu):
    c = small_scene(gpu)
    host = resident(c)
    n = len(host)
    fresh = expected_output(c["files"], c["offsets"], n)
    want, stats, _ = model(host, c["base_vi"], c["base_offsets"], c["vi"], c["offsets"], fresh)
    rs = session(gpu, c)
    bound = rs.in_place_scratch_bound()
    assert bound > 0 and stats[2] > 0
    both = torch.full((n + bound + 64,), FILL, dtype=torch.uint8, device="cuda")
    buf = both[:n]
    buf.copy_(torch.from_numpy(host))
    scratch = torch.full((bound,), 0x3C, dtype=torch.uint8, device="cuda")
    refused(errno.EINVAL, lambda: rs.carry_in_place(None, scratch))
    refused(errno.EINVAL, lambda: rs.carry_in_place(buf, None))
    refused(errno.EINVAL, lambda: rs.carry_in_place(buf, both[n - 16 :]))  # the scratch starts inside the buffer
    refused(errno.EINVAL, lambda: rs.carry_in_place(both[16 : 16 + n], both[:bound]))  # the buffer starts inside the scratch
    refused(errno.ENOMEM, lambda: rs.carry_in_place(buf, scratch[: bound - 1]))
    refused(errno.EINVAL, lambda: rs.carry(buf, buf))  # the out-of-place carry still refuses overlap
    assert rs.finish()[0] == errno.ENOENT
    torch.cuda.synchronize()
    same(buf.cpu().numpy(), host)  # nothing was queued
    rs.carry_in_place(buf, scratch)
    refused(errno.EEXIST, lambda: rs.carry_in_place(buf, scratch))
    refused(errno.EEXIST, lambda: rs.carry(buf, torch.empty(c["out_bytes"], dtype=torch.uint8, device="cuda")))
    elsewhere = torch.full((n,), FILL, dtype=torch.uint8, device="cuda")
    hashes = np.array(c["blocks"], np.uint64)
    refused(errno.EINVAL, lambda: deliver(rs, hashes, c["images"], elsewhere))  # after a carry in place the output is that buffer
    deliver(rs, hashes, c["images"], buf)
    code, res = rs.finish()
    assert code == 0 and res.occurrences_written == res.occurrences
    same(buf.cpu().numpy(), want)
    assert (elsewhere.cpu().numpy() == FILL).all()
    # ---- a blocks call first: the carry in place is refused, and the session completes out of place ----
    rs = session(gpu, c)
    out = torch.full((c["out_bytes"],), FILL, dtype=torch.uint8, device="cuda")
    base = torch.from_numpy(host).cuda()
    deliver(rs, hashes[:1], c["images"][:1], out)
    refused(errno.EINVAL, lambda: rs.carry_in_place(base, scratch))
    rs.carry(base[: c["base_bytes"]], out)
    refused(errno.EEXIST, lambda: rs.carry_in_place(base, scratch))
    deliver(rs, hashes[1:], c["images"][1:], out)
    code, res = rs.finish()
    assert code == 0
    same(out.cpu().numpy(), expected_output(c["files"], c["offsets"], c["out_bytes"]))
    same(base.cpu().numpy(), host)
    # ---- a session without a base ----
    full = Scene(5)
    only = [full.new(100), full.new(200)]
    full.target.append(("f", 3, only))
    p = full.case(gpu, BLK3, [only], 0, 310)
    plain = keep(Restore(gpu, p["vi"], p["si"], p["offsets"], p["out_bytes"], verify=True))
    assert plain.in_place_stats() == (0, 0, 0, 0) and plain.in_place_scratch_bound() == 0
    out = torch.full((310,), FILL, dtype=torch.uint8, device="cuda")
    refused(errno.EINVAL, lambda: plain.carry_in_place(out, scratch))
    deliver(plain, np.array(p["blocks"], np.uint64), p["images"], out)
    assert plain.finish()[0] == 0
    same(out.cpu().numpy(), expected_output(p["files"], p["offsets"], 310))


def test_everything_kept_needs_no_scratch_and_queues_no_copy(gpu):
    c = dict(small_scene(gpu))
    c.update(vi=c["base_vi"], offsets=c["base_offsets"], files=c["base_files"], out_bytes=c["base_bytes"])
    host = resident(c)
    for verify in (False, True):
        rs = session(gpu, c, verify)
        occ = len(occurrences(c["vi"], c["offsets"]))
        assert rs.in_place_stats() == (occ, sum(len(f) for f in c["files"]), 0, 0) and rs.in_place_scratch_bound() == 0
        assert len(rs.needed_blocks()) == 0
        buf = torch.from_numpy(host).cuda()
        gpu.timing(True)
        gpu.timing_reset()
        rs.carry_in_place(buf, None)
        code, res = rs.finish()
        launches = gpu.timing_get()["gather"][1]
        gpu.timing(False)
        assert code == 0 and res.occurrences_written == res.occurrences == occ
        assert launches == 0, "no copy and no run kernel was queued"
        same(buf.cpu().numpy(), host)
    # (the measure itself: a session that moves something does launch in that class)
    moving = small_scene(gpu)
    rs = session(gpu, moving, False)
    gpu.timing(True)
    gpu.timing_reset()
    rs.carry_in_place(torch.from_numpy(resident(moving)).cuda(), torch.empty(rs.in_place_scratch_bound(), dtype=torch.uint8, device="cuda"))
    gpu.sync()
    launches = gpu.timing_get()["gather"][1]
    gpu.timing(False)
    assert launches > 0


# ---- 5. the scratch bound ----


@pytest.mark.parametrize("scene", ["small", "big"])
def test_scratch_of_exactly_the_bound_at_the_end_of_its_allocation(gpu, scene):
    c = small_scene(gpu) if scene == "small" else big_scene(gpu, 40000, False)
    host = resident(c)
    want, stats, _ = model(host, c["base_vi"], c["base_offsets"], c["vi"], c["offsets"], expected_output(c["files"], c["offsets"], len(host)))
    for verify in (False, True):
        code, _, got, rs, guard = update_in_place(gpu, c, host, verify)
        assert code == 0 and rs.in_place_scratch_bound() <= stats[3] + 16 * stats[2] + 64
        same(got, want)
        assert (guard == 0x3C).all(), "nothing is written in front of the scratch"
