"""-m gpu: the repack session (lthip_repack_*, include/longtail_hip.h "the repack session") over the hand-built store of
tests/repack_util.py, whose blocks witness every rule of the session's definitions.

  1. indexes: for percents 0, 1, 50, 99, 100 and the live sets "all", "every second chunk", "one chunk", "none" (and one built to
     witness the rules) the kept index is lthip_get_existing_store_index's bytes, the new index lthip_create_missing_content's on the
     model's moved list, the store index afterwards lthip_store_index_merge(kept under the blocks' own tags, new); the lists are the
     model's
  2. round trip: a version over the live chunks restores, with verify, from the index afterwards and the kept + new images to the bytes a
     restore from the original store gives, and needs no dropped block -- sources in one call, one per call, in reverse order
  3. new blocks of every kind: 4 chunks per block, small blocks, a live list that interleaves tag-0, LZ4 and zstd chunks; every new
     image passes the restore session's check and decodes, a tag-0 image is restore_util.raw_image of its chunks, and where the
     reference is built its reader opens them
  4. the guarantee: a source block -- an LZ4 one, whose chunks are staged, and a raw one, whose chunks go into tag-0 images -- damaged
     in its header, its payload and (verify) one chunk byte; the work buffer behind the blocks calls is compared whole
  5. refusals, each leaving the session usable
  6. writes stay inside: guard bytes around the work buffer, the scratch and the image input of every whole session; a case in which
     the last staged chunk ends at staging_bytes and the last tag-0 chunk at the work buffer's last byte, the guard right behind it
  7. a store the library wrote: a 3 MiB tree in three versions through the stream session against a store, every block as its tag
     says; repacked at 60 % for versions 2 and 3, which then restore byte for byte, while version 1 is refused
  8. allocation failures (the ablation build): create fails with ENOMEM at each allocation in turn, the next create works

Buffers are filled with a pattern first; every comparison is equality."""
import ctypes as C
import errno

import numpy as np
import pytest
import torch

from longtail_amd.lib import (RESTORE_BAD_CHUNK, RESTORE_BAD_HEADER, RESTORE_BAD_PAYLOAD, LongtailHipError, Repack, Restore,
                              store_index_merge)
from tests._libs import have_ref
from tests.archive_util import LZ4, header_bytes, offsets_at_residue, place
from tests.repack_util import BTL1, ZTD1, codec_of_tag, decoded_new_blocks, hand_store, live_sets, model, own_tags, source_block_of
from tests.restore_util import BLK3, block_index_bytes, build_version_index, parse_store_index, raw_image

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 64
PERCENTS = (0, 1, 50, 99, 100)
MAX_BLOCK, MAX_CHUNKS = 1024, 64
_open = []


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    yield
    while _open:
        _open.pop().close()


def keep(obj):
    _open.append(obj)
    return obj


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


def dev_hashes(st, chunks):
    h = np.ascontiguousarray(st["hashes"][list(chunks)], np.uint64) if len(chunks) else np.zeros(0, np.uint64)
    return torch.from_numpy(h.view(np.int64)).cuda() if len(h) else None


@pytest.fixture(scope="module")
def store(oracle, gpu):
    return hand_store(oracle, gpu)


def witness_live(st):
    """All of block 2 (64 raw) and so of its copy, block 14; the shared chunk A and one own chunk of block 11; the shared chunk S, twice,
    and one own chunk each of blocks 12 and 13."""
    b = st["blocks"]
    a, s = st["shared"]
    return list(b[2][2]) + [a, b[11][2][0], s, b[12][2][0], s, b[13][2][1]]


def guarded(nbytes, fill):
    """A device buffer of nbytes with GUARD bytes of another pattern on both sides -> (whole tensor, the view inside)."""
    whole = torch.full((nbytes + 2 * GUARD,), fill ^ 0xFF, dtype=torch.uint8, device="cuda")
    whole[GUARD : GUARD + nbytes] = fill
    return whole, whole[GUARD : GUARD + nbytes]


def guards_intact(whole, nbytes, fill):
    w = whole.cpu().numpy()
    return (w[:GUARD] == fill ^ 0xFF).all() and (w[GUARD + nbytes :] == fill ^ 0xFF).all()


def deliver(rp, st, blocks, work, images=None, checks=None):
    """One lthip_repack_blocks call with these blocks' images, 8-byte aligned, the last ending at the input's last byte, and a scratch of
    exactly the bound, all between guards."""
    imgs = [(images or st["images"])[b] for b in blocks]
    hashes = [int(st["block_hashes"][b]) for b in blocks]
    offs = offsets_at_residue(imgs, 0, 8)
    body = place(imgs, offs)
    whole_b, view_b = guarded(len(body), 0x5A)
    view_b.copy_(dev(body))
    bound = rp.scratch_bound(hashes)
    whole_s, view_s = guarded(bound, 0x3C) if bound else (None, None)
    rp.blocks(hashes, view_b, offs, [len(i) for i in imgs], view_s, work)
    if checks is not None:
        checks.append((whole_b, len(body), 0x5A))
        if bound:
            checks.append((whole_s, bound, None))
    return bound


def run_repack(gpu, st, live_chunks, percent, verify=True, order="one call", max_block=MAX_BLOCK, max_chunks=MAX_CHUNKS, images=None):
    """A whole session -> dict(rp, info, code, new index, result, work (numpy), offsets, sizes, guards ok)."""
    rp = keep(Repack(gpu, st["si"], dev_hashes(st, live_chunks), percent, max_block, max_chunks, verify))
    info = rp.info()
    wb = int(info.work_bytes)
    whole_w, work = guarded(wb, FILL)
    idx = {int(h): b for b, h in enumerate(st["block_hashes"])}
    sources = [idx[int(h)] for h in rp.source_blocks()]
    checks = [(whole_w, wb, FILL)]
    calls = {"one call": [sources], "one per call": [[b] for b in sources], "reverse": [sources[::-1]]}[order]
    for call in calls:
        if call:
            deliver(rp, st, call, work, images, checks)
    before = work.cpu().numpy().copy()  # (behind every blocks call, in front of write: what the scatter alone wrote)
    rp.write(work)
    code, new_index, res = rp.finish()
    ok = all(guards_intact(w, n, f if f is not None else 0x3C) for w, n, f in checks)
    offs, sizes = rp.images() if code == 0 else (None, None)
    return dict(rp=rp, info=info, code=code, new=new_index, res=res, work=work.cpu().numpy(), before=before, offs=offs, sizes=sizes, guards=ok,
                sources=sources)


def restore_version(gpu, vi, si, image_of, verify=True):
    """Restores every asset of vi from si -> (the output bytes, the needed block hashes)."""
    offs, total = Restore.layout(vi, 1)
    rs = keep(Restore(gpu, vi, si, offs, total, verify=verify))
    needed = rs.needed_blocks()
    imgs = [image_of[int(h)] for h in needed]
    ioffs = offsets_at_residue(imgs, 0, 8)
    bound = rs.scratch_bound(needed)
    scratch = torch.full((bound,), 0x3C, dtype=torch.uint8, device="cuda") if bound else None
    out = torch.full((max(total, 1),), FILL, dtype=torch.uint8, device="cuda")
    rs.blocks(needed, dev(place(imgs, ioffs)) if imgs else None, ioffs, [len(i) for i in imgs], scratch, out)
    code, res = rs.finish()
    assert code == 0, (code, res.blocks_bad, res.chunks_mismatched)
    return out.cpu().numpy()[:total], needed


def version_over(st, live_chunks):
    """A VersionIndex whose chunk list is the distinct live chunks: one asset of all of them, one of every third, an empty one."""
    live = list(dict.fromkeys(live_chunks))
    hashes, lens = st["hashes"][live], [st["lens"][c] for c in live]
    assets = [list(range(len(live))), list(range(0, len(live), 3)), []]
    return build_version_index(BLK3, 32768, ["all.bin", "third.bin", "empty.bin"], assets, hashes, lens)


def moved_regions(st, new_index, image_offs):
    """Where every moved chunk goes in the work buffer -> [(first byte, chunk, its source block)]: a tagged new block's chunks back to
    back in the staging region, block after block; a tag-0 block's behind the BlockIndex of its image."""
    p = parse_store_index(new_index)
    by_hash = {int(h): c for c, h in enumerate(st["hashes"])}
    source = source_block_of(st)
    out, staged = [], 0
    for b in range(len(p["block_hashes"])):
        o, n, tag = int(p["block_offsets"][b]), int(p["block_counts"][b]), int(p["block_tags"][b])
        at = staged if tag else int(image_offs[b]) + header_bytes(n, 0)
        for h in p["chunk_hashes"][o : o + n]:
            c = by_hash[int(h)]
            out.append((at, c, source[c]))
            at += st["lens"][c]
        staged = at if tag else staged
    return out


def scattered(st, regions, nbytes, bad_blocks=()):
    """The work buffer as the scatter alone leaves it: the pattern, and every moved chunk of a good source block at its place."""
    buf = np.full(nbytes, FILL, np.uint8)
    for at, c, src in regions:
        if src not in bad_blocks:
            buf[at : at + st["lens"][c]] = st["chunks"][c]
    return buf


def new_images(run):
    return [run["work"][int(o) : int(o) + int(z)].copy() for o, z in zip(run["offs"], run["sizes"])]


# ---- 1. indexes ----


@pytest.mark.parametrize("percent", PERCENTS)
@pytest.mark.parametrize("which", ["all", "every second chunk", "one chunk", "none", "witness"])
def test_indexes_and_lists_are_the_definitions(gpu, store, which, percent):
    st = store
    live = witness_live(st) if which == "witness" else live_sets(st)[which]
    mo = model(st, live, percent)
    d_live = dev_hashes(st, live)
    rp = keep(Repack(gpu, st["si"], d_live, percent, MAX_BLOCK, MAX_CHUNKS, True))
    info = rp.info()
    bh = st["block_hashes"]
    # kept: the call's bytes, and the model's list
    kept = gpu.get_existing_store_index(st["si"], d_live, percent)
    assert rp.kept_index() == kept
    assert list(rp.kept_blocks()) == list(parse_store_index(kept)["block_hashes"]) == [bh[b] for b in mo["kept"]]
    assert list(rp.dropped_blocks()) == [bh[b] for b in mo["dropped"]]
    assert list(rp.source_blocks()) == [bh[b] for b in mo["sources"]]
    # new: lthip_create_missing_content over the model's moved list
    kept_hashes = parse_store_index(kept)["chunk_hashes"]
    d_kept = torch.from_numpy(kept_hashes.view(np.int64)).cuda() if len(kept_hashes) else None
    m = mo["moved"]
    if m:
        want_new = gpu.create_missing_content(d_kept, dev_hashes(st, m), torch.from_numpy(np.array(mo["moved_lens"], np.int32)).cuda(),
                                              mo["moved_tags"], MAX_BLOCK, MAX_CHUNKS)
    else:
        want_new = np.array([1 << 24, 0, 0, 0], np.uint32).tobytes()  # (what the call returns when nothing is missing)
    for b in mo["sources"]:  # (no source carries the unknown tag in these sets)
        assert codec_of_tag(st["blocks"][b][1]) >= 0
    assert (info.blocks_total, info.blocks_kept, info.blocks_dropped, info.blocks_source) == (len(bh), len(mo["kept"]), len(mo["dropped"]),
                                                                                                 len(mo["sources"]))
    assert (info.live_chunks, info.moved_chunks, info.moved_bytes) == (len(mo["live"]), len(m), sum(mo["moved_lens"]))
    for b in mo["sources"]:
        deliver(rp, st, [b], _work(info))
    rp.write(_work(info))
    code, new_index, _ = rp.finish()
    assert code == 0
    assert new_index == want_new
    assert info.new_blocks == len(parse_store_index(want_new)["block_hashes"])
    after = rp.store_index()
    assert after == store_index_merge(own_tags(kept, st["si"]), want_new)
    if own_tags(kept, st["si"]) == kept:
        assert after == store_index_merge(kept, want_new)
    assert (info.kept_index_size, info.new_index_size, info.store_index_size) == (len(kept), len(want_new), len(after))
    if percent == 0:
        assert not m and not mo["sources"], "percent 0 moves nothing"
    if which == "none":
        assert not mo["kept"] and len(mo["dropped"]) == len(bh) and not m, "an empty live set drops everything"
    if which == "witness" and percent == 50:
        a, s = st["shared"]
        assert 2 in mo["kept"] and 11 in mo["dropped"] and a not in m, "a chunk in a kept block and in a victim is not moved"
        assert 12 in mo["dropped"] and 13 in mo["dropped"] and m.count(s) == 1 and 12 in mo["sources"], "a chunk in two victims moves once, from the first"
        assert 14 in mo["dropped"], "a block that passes the threshold but is redundant is not kept"
        assert 15 in mo["dropped"], "a block with no live chunk is not kept"


_work_cache = {}


def _work(info):
    """A work buffer of the plan's size (shared by the index tests, which do not read it)."""
    n = int(info.work_bytes)
    if n not in _work_cache:
        _work_cache[n] = torch.full((max(n, 8),), FILL, dtype=torch.uint8, device="cuda")
    return _work_cache[n]


# ---- 2. round trip ----


@pytest.mark.parametrize("order", ["one call", "one per call", "reverse"])
@pytest.mark.parametrize("which,percent", [("every second chunk", 60), ("all", 100), ("witness", 50)])
def test_round_trip_restores_the_live_chunks(gpu, store, which, percent, order):
    st = store
    live = witness_live(st) if which == "witness" else live_sets(st)[which]
    run = run_repack(gpu, st, live, percent, order=order)
    assert run["code"] == 0 and run["guards"]
    assert run["res"].blocks_bad == 0 and run["res"].chunks_mismatched == 0 and run["res"].blocks_source == len(run["sources"])
    rp = run["rp"]
    # what the scatter alone left: every moved chunk at its place, the pattern everywhere else -- the WHOLE buffer is compared
    regions = moved_regions(st, run["new"], run["offs"])
    assert (run["before"] == scattered(st, regions, int(run["info"].work_bytes))).all()
    after = rp.store_index()
    image_of = {int(h): st["images"][b] for b, h in enumerate(st["block_hashes"])}
    vi = version_over(st, live)
    want, _ = restore_version(gpu, vi, st["si"], image_of)
    dropped = {int(h) for h in rp.dropped_blocks()}
    image_after = {h: i for h, i in image_of.items() if h not in dropped}
    for h, img in zip(parse_store_index(run["new"])["block_hashes"], new_images(run)):
        image_after[int(h)] = img
    got, needed = restore_version(gpu, vi, after, image_after)
    assert (got == want).all()
    assert not dropped & {int(h) for h in needed}
    if which != "all":
        assert run["info"].moved_chunks > 0 and run["info"].new_blocks > 0


# ---- 3. new blocks of every kind ----


def test_new_blocks_of_every_kind(gpu, store):
    st = store
    b = st["blocks"]
    halves = [b[2][2][:32], b[3][2][:32], b[8][2][:10]]  # raw, LZ4, zstd: each about half of its block
    live = [c for trio in zip(*[h[:10] for h in halves]) for c in trio] + halves[0][10:] + halves[1][10:]
    run = run_repack(gpu, st, live, 100, max_block=64, max_chunks=4)
    assert run["code"] == 0 and run["guards"]
    new = parse_store_index(run["new"])
    tags = [int(t) for t in new["block_tags"]]
    assert set(tags) == {0, LZ4, ZTD1} and len(tags) > 12 and max(new["block_counts"]) <= 4
    images = new_images(run)
    expect = decoded_new_blocks(st, run["new"])
    # every new image passes the restore session's check and decodes: a version over the moved chunks, the new index alone
    vi = version_over(st, live)
    got, _ = restore_version(gpu, vi, run["new"], {int(h): i for h, i in zip(new["block_hashes"], images)})
    want, _ = restore_version(gpu, vi, st["si"], {int(h): st["images"][k] for k, h in enumerate(st["block_hashes"])})
    assert (got == want).all()
    for k, (tag, hs, zs, body) in enumerate(expect):
        hdr = header_bytes(len(hs), tag)
        if tag == 0:
            assert len(images[k]) == hdr + len(body) and (images[k] == raw_image(int(new["block_hashes"][k]), BLK3, hs, zs, body)).all(), k
            continue
        # a tagged image: the BlockIndex, then [raw][compressed] that say what the chunks sum to and what lies behind them
        words = np.array([len(body), len(images[k]) - hdr], np.uint32).tobytes()
        assert images[k][:hdr].tobytes() == block_index_bytes(int(new["block_hashes"][k]), BLK3, tag, hs, zs) + words, k
        bound = gpu.lib.dll.lthip_lz4_bound if tag == LZ4 else gpu.lib.dll.lthip_zstd_bound
        assert 0 < len(images[k]) - hdr <= int(bound(len(body))), k
    assert (run["before"] == scattered(st, moved_regions(st, run["new"], run["offs"]), int(run["info"].work_bytes))).all()
    assert run["res"].raw_bytes_written == sum(len(e[3]) for e in expect)
    if have_ref():
        from tests._libs import ref as _ref
        from tests.test_gpu_raw_blocks import ref_opens_raw_image

        r = _ref()
        for k, (tag, hs, zs, body) in enumerate(expect):
            if tag == 0:
                assert ref_opens_raw_image(r, images[k]) == len(body)
                continue
            h, s = np.ascontiguousarray(hs), np.ascontiguousarray(zs)
            out, n = np.zeros(len(body) + 8, np.uint8), C.c_uint64(0)
            err = r.dll.refh_open_stored_block(images[k].ctypes.data, len(images[k]), len(h), h.ctypes.data, s.ctypes.data, tag, out.ctypes.data,
                                               len(body), C.byref(n))
            assert err == 0 and n.value == len(body) and out[: len(body)].tobytes() == body, (k, err)


# ---- 4. the guarantee ----


@pytest.mark.parametrize("victim", [3, 4])  # 64 chunks, LZ4: its chunks are staged; 65 chunks, raw: they go straight into tag-0 images
@pytest.mark.parametrize("damage,verify,flag", [("header", True, RESTORE_BAD_HEADER), ("payload", True, RESTORE_BAD_PAYLOAD),
                                                ("chunk", True, RESTORE_BAD_CHUNK), ("chunk", False, 0)])
def test_no_byte_of_a_bad_block_reaches_the_work_buffer(gpu, store, damage, verify, flag, victim):
    st = store
    live = live_sets(st)["every second chunk"]
    good = run_repack(gpu, st, live, 100, verify=verify)
    assert good["code"] == 0
    assert victim in good["sources"]
    tag = st["blocks"][victim][1]
    images = list(st["images"])
    img = images[victim].copy()
    n = len(st["blocks"][victim][2])
    if damage == "header":
        img[20 + 8 * 5] ^= 1  # a chunk hash
    elif damage == "payload":
        img = img[:-1]  # the literal run is one byte short; a raw image is no longer its BlockIndex and its chunks
        if tag:
            img[header_bytes(n, tag) - 4 : header_bytes(n, tag)] = np.frombuffer(np.uint32(len(img) - header_bytes(n, tag)).tobytes(), np.uint8)
    else:
        img[-3] ^= 0x40  # a byte of the last chunk (literals: the decoder does not notice)
    images[victim] = img
    bad = run_repack(gpu, st, live, 100, verify=verify, images=images)
    rp = bad["rp"]
    status = rp.block_status([int(st["block_hashes"][victim])])
    if not flag:  # without verify the chunk byte goes through, as in the restore session
        assert bad["code"] == 0 and status[0] == 0
        return
    assert bad["code"] == errno.EBADF and bad["new"] is None and bad["res"].blocks_bad == 1
    assert status[0] == flag
    for call in (rp.images, rp.store_index):
        with pytest.raises(LongtailHipError) as e:
            call()
        assert e.value.code == errno.EBADF
    # The plan is the good run's.  Behind the blocks calls the WHOLE work buffer is compared: the destinations the bad block would have
    # fed still hold the pattern, every other moved chunk is where the good run put it, nothing else was written.
    wb = int(good["info"].work_bytes)
    regions = moved_regions(st, good["new"], good["offs"])
    fed = [(at, c) for at, c, src in regions if src == victim]
    assert len(fed) > 10
    if tag == 0:
        assert all(at >= int(good["info"].staging_bytes) for at, _ in fed), "a raw source's chunks go into the image region"
    assert (good["before"] == scattered(st, regions, wb)).all()
    assert (bad["before"] == scattered(st, regions, wb, bad_blocks={victim})).all()
    # ... and write changed none of that: no byte of the bad block in the buffer as it was left
    for at, c in fed:
        assert (bad["work"][at : at + st["lens"][c]] == FILL).all(), c
    assert bad["guards"]


# ---- 5. refusals ----


def test_refusals_leave_the_session_usable(gpu, store):
    st = store
    live = live_sets(st)["every second chunk"]
    rp = keep(Repack(gpu, st["si"], dev_hashes(st, live), 100, MAX_BLOCK, MAX_CHUNKS, True))
    info = rp.info()
    work = torch.full((int(info.work_bytes),), FILL, dtype=torch.uint8, device="cuda")
    idx = {int(h): b for b, h in enumerate(st["block_hashes"])}
    sources = [idx[int(h)] for h in rp.source_blocks()]
    assert len(sources) > 4

    def refused(code, fn, *args):
        with pytest.raises(LongtailHipError) as e:
            fn(*args)
        assert e.value.code == code, (e.value.code, code)

    first, rest = sources[:2], sources[2:]
    # a work buffer that is not 8-byte aligned: refused by both calls, before anything else is looked at
    askew = torch.full((int(info.work_bytes) + 8,), FILL, dtype=torch.uint8, device="cuda")[4:]
    assert askew.data_ptr() % 8 == 4 and work.data_ptr() % 8 == 0
    img0, h0 = st["images"][first[0]], int(st["block_hashes"][first[0]])
    refused(errno.EINVAL, rp.blocks, [h0], dev(place([img0], [0])), [0], [len(img0)], torch.zeros(max(rp.scratch_bound([h0]), 8), dtype=torch.uint8,
                                                                                                    device="cuda"), askew)
    refused(errno.EINVAL, rp.write, askew)
    deliver(rp, st, first, work)
    refused(errno.ENOENT, rp.write, work)  # sources are outstanding: nothing queued
    assert rp.finish()[0] == errno.ENOENT
    img = st["images"][rest[0]]
    body, h = dev(place([img], [0])), int(st["block_hashes"][rest[0]])
    scratch = torch.zeros(max(rp.scratch_bound([h]), 8), dtype=torch.uint8, device="cuda")
    refused(errno.ENOENT, rp.blocks, [0x1234], body, [0], [len(img)], scratch, work)
    refused(errno.EEXIST, rp.blocks, [int(st["block_hashes"][first[0]])], body, [0], [len(img)], scratch, work)
    refused(errno.EEXIST, rp.blocks, [h, h], body, [0, 0], [len(img)] * 2, scratch, work)
    refused(errno.EINVAL, rp.blocks, [h], dev(place([img], [4])), [4], [len(img)], scratch, work)
    tagged = [b for b in rest if st["blocks"][b][1]]
    ht = int(st["block_hashes"][tagged[0]])
    bound = rp.scratch_bound([ht])
    assert bound > 0
    refused(errno.ENOMEM, rp.blocks, [ht], dev(place([st["images"][tagged[0]]], [0])), [0], [len(st["images"][tagged[0]])],
            torch.zeros(bound - 1, dtype=torch.uint8, device="cuda"), work)
    # a block that is no source is accepted, counted and not touched
    kept_or_idle = [b for b in range(len(st["blocks"])) if b not in sources][0]
    deliver(rp, st, [kept_or_idle], work)
    deliver(rp, st, rest, work)
    rp.write(work)
    refused(errno.EEXIST, rp.write, work)
    code, new_index, res = rp.finish()
    assert code == 0 and res.blocks_delivered == len(sources) + 1 and res.blocks_source == len(sources)
    assert new_index == run_repack(gpu, st, live, 100)["new"]


def test_create_refusals(gpu, store):
    st = store
    live = live_sets(st)["all"]

    def refused(code, *args, **kw):
        with pytest.raises(LongtailHipError) as e:
            keep(Repack(gpu, *args, **kw))
        assert e.value.code == code, (e.value.code, code)

    refused(errno.EINVAL, st["si"], dev_hashes(st, live), 101, MAX_BLOCK, MAX_CHUNKS)
    refused(errno.EINVAL, st["si"], dev_hashes(st, live), 50, 0, MAX_CHUNKS)
    refused(errno.EINVAL, st["si"], dev_hashes(st, live), 50, MAX_BLOCK, 0)
    refused(errno.EBADF, st["si"][:-1], dev_hashes(st, live), 50, MAX_BLOCK, MAX_CHUNKS)
    unknown = torch.from_numpy(np.array([int(st["hashes"][0]), 0x1234567], np.uint64).view(np.int64)).cuda()
    refused(errno.ENOENT, st["si"], unknown, 50, MAX_BLOCK, MAX_CHUNKS)
    # the unknown tag: fine on a kept block and on a dropped block that is no source, ENOTSUP when the block is a source
    u = st["blocks"][st["unknown_block"]][2]
    assert st["blocks"][st["unknown_block"]][1] == BTL1
    keep(Repack(gpu, st["si"], dev_hashes(st, u), 100, MAX_BLOCK, MAX_CHUNKS))  # all of it is live: kept
    keep(Repack(gpu, st["si"], dev_hashes(st, live_sets(st)["one chunk"]), 100, MAX_BLOCK, MAX_CHUNKS))  # dropped, no source
    refused(errno.ENOTSUP, st["si"], dev_hashes(st, u[:1]), 100, MAX_BLOCK, MAX_CHUNKS)
    # ... and the context stays usable
    assert run_repack(gpu, st, live_sets(st)["one chunk"], 100)["code"] == 0


# ---- 6. writes stay inside ----


def summing_to_a_multiple_of_8(st, chunks, count):
    """The first `count` of these chunks, in their order, whose sizes sum to a multiple of 8."""
    import itertools

    for combo in itertools.combinations(chunks[:14], count):
        if sum(st["lens"][c] for c in combo) % 8 == 0:
            return list(combo)
    raise AssertionError("no such combination among these chunks")


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("order", ["staged then raw", "staged only"])
def test_the_last_chunk_of_a_region_ends_at_its_last_byte(gpu, store, order, verify):
    """No slack hides an overrun of the scatter's 16-byte stores.  The staged chunks sum to a multiple of 8, so the last of them ends
    at staging_bytes and the first image's BlockIndex follows it directly; the last new block is tag 0 with three chunks (a BlockIndex
    of 56 bytes) that sum to a multiple of 8, so its last chunk's last byte is the work buffer's last byte and the guard follows it
    directly.  The buffer is compared whole behind the blocks calls, and the images after write."""
    st = store
    b = st["blocks"]
    staged = summing_to_a_multiple_of_8(st, b[3][2][1:], 5)  # LZ4 chunks
    tail = summing_to_a_multiple_of_8(st, b[2][2][20:], 3) if order == "staged then raw" else []  # tag-0 chunks (not the shared one)
    run = run_repack(gpu, st, staged + tail, 100, verify=verify, max_block=4096, max_chunks=64)
    assert run["code"] == 0
    info, new = run["info"], parse_store_index(run["new"])
    wb = int(info.work_bytes)
    assert [int(t) for t in new["block_tags"]] == ([LZ4, 0] if tail else [LZ4])
    regions = moved_regions(st, run["new"], run["offs"])
    ends = [at + st["lens"][c] for at, c, _ in regions]
    assert int(info.staging_bytes) == sum(st["lens"][c] for c in staged) == ends[len(staged) - 1] == int(run["offs"][0])
    if tail:
        assert ends[-1] == int(run["offs"][-1]) + int(run["sizes"][-1]) == wb, "the last chunk's last byte is the work buffer's"
    assert (run["before"] == scattered(st, regions, wb)).all()
    assert run["guards"]
    images, expect = new_images(run), decoded_new_blocks(st, run["new"])
    tag, hs, zs, body = expect[0]
    hdr = header_bytes(len(hs), tag)
    words = np.array([len(body), len(images[0]) - hdr], np.uint32).tobytes()
    assert images[0][:hdr].tobytes() == block_index_bytes(int(new["block_hashes"][0]), BLK3, tag, hs, zs) + words
    assert run["work"][: int(info.staging_bytes)].tobytes() == body, "write reads the staged bytes and leaves them"
    if tail:
        _, hs, zs, body = expect[1]
        assert (images[1] == raw_image(int(new["block_hashes"][1]), BLK3, hs, zs, body)).all()
    # ... and the images restore
    vi = version_over(st, staged + tail)
    got, _ = restore_version(gpu, vi, run["new"], {int(h): i for h, i in zip(new["block_hashes"], images)})
    assert got[: len(b"".join(st["chunks"][c].tobytes() for c in staged + tail))].tobytes() == b"".join(st["chunks"][c].tobytes() for c in staged + tail)


# ---- 7. a store the library wrote ----

NFILES, FILE_BYTES, TARGET = 48, 65536, 4096


def ingest_version(gpu, oracle, files, tags, store):
    """The tree of `files` through the stream session in one slice, every block as its tag says, against `store` (or none)
    -> (vi, si, {block hash: image})."""
    from longtail_amd.lib import Ingest, IngestStream, chunker_params

    n = len(files)
    names = [f"dir{i % 4}/file{i:03d}.bin" for i in range(n)]
    path_data = ("\0".join(names) + "\0").encode()
    path_offs = np.concatenate([[0], np.cumsum([len(s) + 1 for s in names])[:-1]]).astype(np.uint32)
    sizes = np.full(n, FILE_BYTES, np.uint64)
    tree, _keep = Ingest.tree(sizes, path_offs, np.full(n, 0o644, np.uint16), path_data, np.arange(n, dtype=np.uint32), np.zeros(n + 1, np.uint64),
                              asset_tags=tags)
    data = torch.from_numpy(np.concatenate(files + [np.zeros(256, np.uint8)])).cuda()
    mn, av, mx = chunker_params(TARGET)
    plan = gpu.make_plan(np.arange(n, dtype=np.uint64) * FILE_BYTES, sizes, mn, av, mx)
    total, d_off, d_len, d_hash, d_first = gpu.chunk_hash(plan, data)
    st = keep(IngestStream(gpu, tree, TARGET, 262144, 64, "by-tag"))  # (a block holds about four files of one tag)
    if store is not None:
        st.set_store(store)
    arena = torch.zeros(max(64, st.arena_bound(n * FILE_BYTES, total)), dtype=torch.uint8, device="cuda")
    tail = torch.zeros(st.arena_bound(0, 0), dtype=torch.uint8, device="cuda")
    st.slice(0, n, data, d_off, d_len, d_hash, d_first, total, arena)
    _, offs0, sizes0 = st.images()
    vi_cap = int(gpu.lib.dll.lthip_version_index_size(n, total, total, len(path_data))) + 64
    h_vi, h_si = torch.zeros(vi_cap, dtype=torch.uint8).pin_memory(), torch.zeros(16 + 32 * max(total, 1) + 64, dtype=torch.uint8).pin_memory()
    res = st.finish(tail, h_vi, h_si)
    _, offs1, sizes1 = st.images()
    vi, si = bytes(h_vi.numpy()[: res.version_index_size]), bytes(h_si.numpy()[: res.store_index_size])
    plan.close()
    hashes = parse_store_index(si)["block_hashes"]
    a, t = arena.cpu().numpy(), tail.cpu().numpy()
    images = [a[int(o) : int(o) + int(z)].copy() for o, z in zip(offs0, sizes0)] + [t[int(o) : int(o) + int(z)].copy() for o, z in zip(offs1, sizes1)]
    assert len(images) == len(hashes)
    return vi, si, {int(h): i for h, i in zip(hashes, images)}


def test_a_store_the_library_wrote(gpu, oracle):
    from longtail_amd.lib import Store, version_chunk_hashes

    v1 = [oracle.synth(FILE_BYTES, 900 + i, (1, 0, 2)[i % 3]) for i in range(NFILES)]
    # (a block ends where the tag changes, so the tags come in thirds; a block holds about four files, and version 2 replaces two of
    # every four among the first 24: those blocks of version 1 stay half live)
    v2 = [oracle.synth(FILE_BYTES, 2000 + i, (1, 0, 2)[i % 3]) if i < 24 and i % 4 < 2 else f for i, f in enumerate(v1)]
    v3 = [oracle.synth(FILE_BYTES, 3000 + i, (1, 0, 2)[i % 3]) if 8 <= i < 32 and i % 4 == 2 else f for i, f in enumerate(v2)]
    tags = np.array([(0, LZ4, 0x7A746432)[i * 3 // NFILES] for i in range(NFILES)], np.uint32)
    known = keep(Store(gpu, 0))
    vis, si_all, image_of = [], None, {}
    for files in (v1, v2, v3):
        vi, si, images = ingest_version(gpu, oracle, files, tags, known if vis else None)
        known.add_index(si)
        vis.append(vi)
        si_all = si if si_all is None else store_index_merge(si_all, si)
        image_of.update(images)
    live = np.concatenate([version_chunk_hashes(vis[1]), version_chunk_hashes(vis[2])])
    rp = keep(Repack(gpu, si_all, torch.from_numpy(live.view(np.int64)).cuda(), 60, 65536, 64, True))
    info = rp.info()
    shape = {k: int(getattr(info, k)) for k in ("blocks_total", "blocks_kept", "blocks_dropped", "blocks_source", "moved_chunks", "new_blocks")}
    assert info.moved_chunks > 0 and info.blocks_dropped >= info.blocks_source > 0 and info.new_blocks > 0, f"the case moves nothing: {shape}"
    assert {int(t) for t in parse_store_index(si_all)["block_tags"]} == {0, LZ4, 0x7A746432}, "the store holds blocks of every kind"
    work = torch.full((int(info.work_bytes),), FILL, dtype=torch.uint8, device="cuda")
    sources = [int(h) for h in rp.source_blocks()]
    imgs = [image_of[h] for h in sources]
    offs = offsets_at_residue(imgs, 0, 8)
    bound = rp.scratch_bound(sources)
    scratch = torch.zeros(max(bound, 8), dtype=torch.uint8, device="cuda")
    rp.blocks(sources, dev(place(imgs, offs)), offs, [len(i) for i in imgs], scratch, work)
    rp.write(work)
    code, new_index, res = rp.finish()
    assert code == 0 and res.blocks_bad == 0 and res.raw_bytes_written == info.moved_bytes
    after = rp.store_index()
    dropped = {int(h) for h in rp.dropped_blocks()}
    offs_new, sizes_new = rp.images()
    host = work.cpu().numpy()
    image_after = {h: i for h, i in image_of.items() if h not in dropped}
    for h, o, z in zip(parse_store_index(new_index)["block_hashes"], offs_new, sizes_new):
        image_after[int(h)] = host[int(o) : int(o) + int(z)].copy()
    assert len(after) < len(si_all)
    for vi, files in ((vis[1], v2), (vis[2], v3)):
        got, needed = restore_version(gpu, vi, after, image_after)
        assert (got == np.concatenate(files)).all()
        assert not dropped & {int(h) for h in needed}
    offs1, total1 = Restore.layout(vis[0], 1)
    with pytest.raises(LongtailHipError) as e:  # version 1 was not kept: the store no longer holds all of it
        keep(Restore(gpu, vis[0], after, offs1, total1, verify=True))
    assert e.value.code == errno.ENOENT


# ---- 8. allocation failures ----


def test_create_enomem_at_each_allocation_then_recovers(gpu, gpu_abl, store):
    st = store
    d = gpu_abl.lib.dll
    assert d.lthip_debug_fail_alloc(-1, 0) == 0, "the ablation build must have the injection switch"
    live = live_sets(st)["every second chunk"]

    def create():
        return Repack(gpu_abl, st["si"], dev_hashes(st, live), 100, MAX_BLOCK, MAX_CHUNKS)

    def calls():
        return int(d.lthip_debug_alloc_calls(None))

    # the context's pools and its ring of staging slots grow over the first sessions: until two creates in a row allocate the same
    counts = []
    for _ in range(80):
        n0 = calls()
        want = create()
        counts.append(calls() - n0)
        kept, sources = list(want.kept_blocks()), list(want.source_blocks())
        want.close()
        if len(counts) >= 3 and counts[-1] == counts[-2] == counts[-3]:
            break
    n = counts[-1]
    assert counts[-1] == counts[-2] == counts[-3] and n > 10, counts
    try:
        for k in range(n):
            d.lthip_debug_fail_alloc(k, 1 << 60)
            try:
                err = 0
                try:
                    create().close()
                except LongtailHipError as e:
                    err = e.code
                assert err == errno.ENOMEM, f"allocation {k + 1} of {n} failing gave errno {err}"
            finally:
                d.lthip_debug_fail_alloc(-1, 0)
            again = create()  # the next create on the same context works
            assert list(again.kept_blocks()) == kept and list(again.source_blocks()) == sources
            again.close()
    finally:
        d.lthip_debug_fail_alloc(-1, 0)
