"""-m gpu: the restore session (lthip_restore_*, include/longtail_hip.h) -- stored-block images back into a version's assets.

  * an alignment sweep on a version built by hand: every chunk length of a list at every destination residue mod 16, source residues
    mod 4 all met, every chunk used by many assets
  * round trips of what the stream ingest session wrote (tests/test_gpu_ingest_stream.py's trees and run_stream, cut per job): raw, LZ4,
    zstd and by-tag images, 'blk3', 'blk2' and 'meow' chunk hashes -- every asset's window equals the file
  * any batching of the blocks gives the same output; finish before the last batch says how many blocks are outstanding
  * a partial restore (every second asset) writes nothing outside the selected windows
  * a store whose tagged payloads the REFERENCE's codecs wrote restores to the same files
  * damaged headers and raw blocks: the block is flagged, nothing of it reaches the output, everything else is right
  * refusals leave the context and the session usable
  * lthip_seen_find against a Python dict

In every test the output buffer is filled with 0xA5 first and compared WHOLE with what is expected.  Every comparison is equality."""
import errno

import numpy as np
import pytest
import torch

from longtail_amd.lib import (RESTORE_BAD_CHUNK, RESTORE_BAD_HEADER, RESTORE_NOT_DELIVERED, LongtailHipError, Restore, Seen)
from tests.gpu_util import dev_u64
from tests.restore_util import (BLK2, BLK3, MEOW, build_store_index, build_version_index, numpy_layout, parse_store_index,
                                parse_version_index, raw_image, without_last_block)
from tests.test_gpu_ingest_by_tag import CONFIGS, LZ4, ZTD2, ZTD4, rotating_tags
from tests.test_gpu_ingest_stream import _sessions, chunk_jobs, index_buffers, open_stream, run_stream, slices_of, stream_tree, tree_of

pytestmark = pytest.mark.gpu

FILL = 0xA5
_open, _runs = [], {}


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


# ---- what the stream session wrote, once per configuration ----


def run_meow(ctx, tree, target, codec, max_block, max_chunks, tag, cuts):
    """run_stream with Meow chunk hashes (its chunk_jobs knows 'blk3' and 'blk2')."""
    st = open_stream(ctx, stream_tree(tree, None), target, max_block, max_chunks, codec, compression_type=tag, hash_identifier=MEOW)
    calls, chunks_all = [], 0

    def take(arena):
        first, offs, sizes = st.images()
        host = arena.cpu().numpy()
        calls.append((first, [host[int(o) : int(o) + int(n)].copy() for o, n in zip(offs, sizes)]))

    for first_job, count in cuts:
        sl = chunk_jobs(ctx, tree, target, first_job, count)
        bound = max(1, int(sl["d_hash"].numel()))
        ctx.meow_ranges(sl["dev"], sl["d_off"], sl["d_len"], out=sl["d_hash"], count_bound=bound, d_count=sl["d_first"][count : count + 1])
        arena = torch.zeros(max(64, st.arena_bound(sl["bytes"], sl["total"])), dtype=torch.uint8, device="cuda")
        st.slice(first_job, count, sl["dev"], sl["d_off"], sl["d_len"], sl["d_hash"], sl["d_first"], sl["total"], arena)
        take(arena)
        chunks_all += sl["total"]
    arena = torch.zeros(st.arena_bound(0, 0), dtype=torch.uint8, device="cuda")
    vi, si = index_buffers(ctx, tree, chunks_all)
    res = st.finish(arena, vi, si)
    take(arena)
    return dict(st=st, res=res, vi=bytes(vi.numpy()[: res.version_index_size]), si=bytes(si.numpy()[: res.store_index_size]), calls=calls)


def written(gpu, oracle, ref, codec, cfg, hash_id=BLK3):
    """The session's index pair and images for the tree, cut per job: dict(tree, vi, si, images (StoreIndex order), blocks)."""
    key = (codec, cfg, hash_id)
    if key not in _runs:
        target, max_block, max_chunks = cfg
        tree = tree_of(oracle, ref, target)
        cuts = slices_of("per-job", tree["part"].job_count)
        tag = {"none": None, "lz4": LZ4, "zstd": ZTD2, "by-tag": None}[codec]
        if hash_id == MEOW:
            run = run_meow(gpu, tree, target, codec, max_block, max_chunks, tag, cuts)
        else:
            tags = rotating_tags(tree, (0, LZ4, ZTD2, ZTD4)) if codec == "by-tag" else None
            run = run_stream(gpu, tree, target, codec, max_block, max_chunks, tag, cuts, asset_tags=tags, hash_id=hash_id, scribble=False)
        images = [i for _, imgs in run["calls"] for i in imgs]
        assert len(images) == run["res"].blocks == len(parse_store_index(run["si"])["block_hashes"]) > 0
        _runs[key] = dict(tree=tree, vi=run["vi"], si=run["si"], images=images, blocks=run["res"].blocks)
        while _sessions:
            _sessions.pop().close()
    return _runs[key]


def files_of(tree):
    return [tree["by_name"].get(p, np.zeros(0, np.uint8)) for p in tree["paths"]]


def expected_output(files, offsets, out_bytes):
    out = np.full(out_bytes, FILL, np.uint8)
    for data, off in zip(files, offsets):
        if int(off) != Restore.SKIP and len(data):
            out[int(off) : int(off) + len(data)] = data
    return out


def pack(images):
    """The images back to back at 8-byte aligned offsets, the last one ending at the buffer's last byte."""
    offs, at = [], 0
    for i in images:
        at = (at + 7) // 8 * 8
        offs.append(at)
        at += len(i)
    host = np.full(max(at, 1), 0x5A, np.uint8)
    for o, i in zip(offs, images):
        host[o : o + len(i)] = i
    return torch.from_numpy(host).cuda(), np.array(offs, np.uint64), np.array([len(i) for i in images], np.uint32)


def deliver(rs, hashes, images, out, scratch_extra=0):
    """One lthip_restore_blocks call with scratch of exactly lthip_restore_scratch_bound (+ scratch_extra) bytes."""
    dev, offs, sizes = pack(images)
    bound = rs.scratch_bound(hashes) + scratch_extra
    scratch = torch.full((bound,), 0x3C, dtype=torch.uint8, device="cuda") if bound > 0 else None
    rs.blocks(hashes, dev, offs, sizes, scratch, out)


def restore(gpu, vi, si, images, offsets, out_bytes, verify=True, batches=None):
    """-> (finish's code, the result, the output, the session).  batches: lists of block indices, one call each (default: one call)."""
    block_hashes = parse_store_index(si)["block_hashes"]
    rs = keep(Restore(gpu, vi, si, offsets, out_bytes, verify=verify))
    out = torch.full((max(out_bytes, 1),), FILL, dtype=torch.uint8, device="cuda")
    for batch in [list(range(len(images)))] if batches is None else batches:
        deliver(rs, block_hashes[batch], [images[b] for b in batch], out)
    code, res = rs.finish()
    return code, res, out.cpu().numpy()[:out_bytes], rs


def occurrences(vi, offsets):
    """(chunk hash, destination, length) of every chunk of every selected asset."""
    p = parse_version_index(vi)
    occ = []
    for a, off in enumerate(offsets):
        if int(off) == Restore.SKIP:
            continue
        at = int(off)
        for c in p["idx"][int(p["starts"][a]) : int(p["starts"][a]) + int(p["counts"][a])]:
            occ.append((int(p["chunk_hashes"][c]), at, int(p["chunk_sizes"][c])))
            at += int(p["chunk_sizes"][c])
    return occ


# ---- 1. the alignment sweep ----

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 63, 255, 4097]


def test_every_length_at_every_alignment(gpu, oracle):
    """One raw block of 16 chunks; 16 assets that each hold all 16 chunks, asset r at r * 8192 + r: chunk j lands at destination residue
    (r + the lengths before it) mod 16, so every length meets every residue, and every chunk is used by 16 assets (more than the three
    the dedup needs).  The payload starts 212 bytes into an 8-aligned image, so a chunk's source residue mod 4 is that of the lengths
    before it: all four occur."""
    rng = np.random.default_rng(9)
    chunks = [rng.integers(0, 256, n).astype(np.uint8) for n in LENGTHS]
    content = np.concatenate(chunks)
    starts = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    hashes = oracle.blake3_many(content, starts, LENGTHS)
    block_hash = oracle.blake3(np.frombuffer(hashes.tobytes(), np.uint8))
    n = len(LENGTHS)
    names = [f"a{r:02d}" for r in range(16)]
    vi = build_version_index(BLK3, 32768, names, [list(range(n))] * 16, hashes, LENGTHS)
    si = build_store_index(BLK3, [(block_hash, 0, list(range(n)))], hashes, LENGTHS)
    offsets = np.array([r * 8192 + r for r in range(16)], np.uint64)
    out_bytes = 16 * 8192
    for j in range(n):
        assert {(int(o) + int(starts[j])) % 16 for o in offsets} == set(range(16))
    image = raw_image(block_hash, BLK3, hashes, LENGTHS, content)
    code, res, out, _ = restore(gpu, vi, si, [image], offsets, out_bytes, verify=True)
    assert code == 0
    want = expected_output([content] * 16, offsets, out_bytes)
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])
    assert res.occurrences == res.occurrences_written == 16 * n and res.bytes_written == 16 * len(content)
    assert (res.assets_selected, res.blocks_needed, res.blocks_delivered, res.blocks_bad, res.chunks_mismatched) == (16, 1, 1, 0, 0)


# ---- 2. round trips ----

ROUND_TRIPS = [(codec, cfg, BLK3) for codec in ("none", "lz4", "zstd", "by-tag") for cfg in CONFIGS] + [("lz4", CONFIGS[1], BLK2), ("zstd", CONFIGS[1], MEOW)]


def check_round_trip(gpu, w, batches=None, verify=True):
    files = files_of(w["tree"])
    offsets, total = Restore.layout(w["vi"], 64)
    want_offsets, want_total = numpy_layout([len(f) for f in files], 64)
    assert (offsets == want_offsets).all() and total == want_total
    code, res, out, rs = restore(gpu, w["vi"], w["si"], w["images"], offsets, total, verify=verify, batches=batches)
    assert code == 0
    want = expected_output(files, offsets, total)
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])
    assert res.bytes_written == sum(len(f) for f in files)
    assert res.blocks_delivered == w["blocks"] == res.blocks_needed and res.blocks_unneeded == res.blocks_bad == res.chunks_mismatched == 0
    assert res.occurrences_written == res.occurrences > 0 and res.assets_selected == len(files)
    assert (rs.block_status(parse_store_index(w["si"])["block_hashes"]) == 0).all()
    return res


@pytest.mark.parametrize("codec,cfg,hash_id", ROUND_TRIPS)
def test_the_sessions_own_images_restore_to_the_files(gpu, oracle, ref, codec, cfg, hash_id):
    w = written(gpu, oracle, ref, codec, cfg, hash_id)
    assert parse_version_index(w["vi"])["hash_id"] == hash_id
    res = check_round_trip(gpu, w)
    tags = parse_store_index(w["si"])["block_tags"]
    if codec == "none":
        assert res.decoded_bytes == 0 and (tags == 0).all()
    elif codec == "by-tag":
        assert len(set(tags.tolist())) >= 3 and 0 in tags, "raw, LZ4 and zstd blocks in one call"
        assert 0 < res.decoded_bytes < res.bytes_written
    else:
        assert res.decoded_bytes > 0


# ---- 3. any batching ----


def test_any_batching_gives_the_same_output(gpu, oracle, ref):
    w = written(gpu, oracle, ref, "by-tag", CONFIGS[1])
    nb = w["blocks"]
    assert nb >= 6
    check_round_trip(gpu, w, batches=[[b] for b in reversed(range(nb))])
    order = np.random.default_rng(4).permutation(nb)
    batches = [order[k::3].tolist() for k in range(3)]
    # ---- three shuffled batches; finish before the last one ----
    files = files_of(w["tree"])
    offsets, total = Restore.layout(w["vi"], 64)
    hashes = parse_store_index(w["si"])["block_hashes"]
    rs = keep(Restore(gpu, w["vi"], w["si"], offsets, total, verify=True))
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    for batch in batches[:2]:
        deliver(rs, hashes[batch], [w["images"][b] for b in batch], out)
    code, res = rs.finish()
    assert code == errno.ENOENT
    assert res.blocks_needed - (res.blocks_delivered - res.blocks_unneeded) == len(batches[2]) and res.blocks_bad == 0
    st = rs.block_status(hashes)
    assert (st[batches[2]] == RESTORE_NOT_DELIVERED).all() and (st[batches[0] + batches[1]] == 0).all()
    deliver(rs, hashes[batches[2]], [w["images"][b] for b in batches[2]], out)
    code, res = rs.finish()
    assert code == 0 and res.blocks_delivered == nb and res.bytes_written == sum(len(f) for f in files)
    want = expected_output(files, offsets, total)
    got = out.cpu().numpy()
    assert (got == want).all(), int(np.flatnonzero(got != want)[0])


# ---- 4. a partial restore ----


def test_a_partial_restore_writes_the_selected_windows_only(gpu, oracle, ref):
    w = written(gpu, oracle, ref, "by-tag", CONFIGS[0])
    files = files_of(w["tree"])
    selected = [a % 2 == 0 for a in range(len(files))]
    offs, total = numpy_layout([len(f) if s else 0 for f, s in zip(files, selected)], 1)  # dense: no gap, no alignment
    offsets = np.array([int(o) if s else Restore.SKIP for o, s in zip(offs, selected)], np.uint64)
    assert total == sum(len(f) for f, s in zip(files, selected) if s) > 0
    pad = 4096  # room behind the windows that must stay untouched
    hashes = parse_store_index(w["si"])["block_hashes"]
    index_of = {int(h): b for b, h in enumerate(hashes)}
    rs = keep(Restore(gpu, w["vi"], w["si"], offsets, total, verify=True))
    needed = rs.needed_blocks()
    assert 0 < len(needed) < len(hashes) and all(int(h) in index_of for h in needed)
    assert [index_of[int(h)] for h in needed] == sorted(index_of[int(h)] for h in needed), "StoreIndex order"
    out = torch.full((total + pad,), FILL, dtype=torch.uint8, device="cuda")
    deliver(rs, needed, [w["images"][index_of[int(h)]] for h in needed], out)
    code, res = rs.finish()
    assert code == 0 and res.blocks_delivered == res.blocks_needed == len(needed) and res.blocks_unneeded == 0
    extra = next(b for b, h in enumerate(hashes) if int(h) not in set(int(x) for x in needed))
    assert rs.scratch_bound(hashes[[extra]]) == 0
    deliver(rs, hashes[[extra]], [w["images"][extra]], out)
    code, res = rs.finish()
    assert code == 0 and res.blocks_delivered == len(needed) + 1 and res.blocks_unneeded == 1
    assert res.assets_selected == sum(selected) and res.bytes_written == total
    want = expected_output(files, offsets, total + pad)
    got = out.cpu().numpy()
    assert (got == want).all(), int(np.flatnonzero(got != want)[0])


# ---- 5. a store the reference's codecs wrote ----


def test_a_store_the_reference_wrote_restores_to_the_files(gpu, oracle, ref):
    w = written(gpu, oracle, ref, "by-tag", CONFIGS[1])
    files = files_of(w["tree"])
    offsets, total = Restore.layout(w["vi"], 64)
    si = parse_store_index(w["si"])
    # the chunks' bytes, from the files (through the expected output: chunk h lies wherever an occurrence of it lands)
    want = expected_output(files, offsets, total)
    where = {h: want[at : at + n] for h, at, n in occurrences(w["vi"], offsets)}
    images, met = [], set()
    for b, image in enumerate(w["images"]):
        c0, n, tag = int(si["block_offsets"][b]), int(si["block_counts"][b]), int(si["block_tags"][b])
        if tag == 0:
            images.append(image)
            continue
        parts = [where[int(h)] for h in si["chunk_hashes"][c0 : c0 + n]]
        content = np.ascontiguousarray(np.concatenate(parts))
        payload = ref.compress(0 if tag == LZ4 else 1, tag, content)
        words = np.array([len(content), len(payload)], np.uint32).view(np.uint8)
        images.append(np.concatenate([image[: gpu.block_index_size(n)], words, payload]))
        met.add(tag)
    assert len(met) >= 2, "LZ4 and zstd payloads of the reference"
    code, res, out, _ = restore(gpu, w["vi"], w["si"], images, offsets, total, verify=True)
    assert code == 0 and res.blocks_bad == 0
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])


# ---- 6. damage (headers and raw blocks only: the decoders' verdicts on damaged payloads are tests/test_gpu_codecs.py's) ----


def damaged_case(w, case):
    """-> (images with one of them damaged, the bad block, the flag it must carry)"""
    si = parse_store_index(w["si"])
    images = [i.copy() for i in w["images"]]
    tags = si["block_tags"]
    if case == "chunk hash bit":
        b = int(np.flatnonzero(tags == LZ4)[0])
        images[b][20 + 3] ^= 0x10
        return images, b, RESTORE_BAD_HEADER
    if case == "raw size word":
        b = int(np.flatnonzero(tags != 0)[-1])
        o = 20 + 12 * int(si["block_counts"][b])
        images[b][o : o + 4] = (images[b][o : o + 4].view(np.uint32) + 1).view(np.uint8)
        return images, b, RESTORE_BAD_HEADER
    raw = np.flatnonzero(tags == 0)
    if case == "another block's image":
        b, other = int(raw[0]), int(raw[1])
        images[b] = w["images"][other].copy()
        return images, b, RESTORE_BAD_HEADER
    b = int(raw[len(raw) // 2])  # "content byte"
    images[b][20 + 12 * int(si["block_counts"][b]) + 5] ^= 0x01
    return images, b, RESTORE_BAD_CHUNK


@pytest.mark.parametrize("case", ["chunk hash bit", "raw size word", "another block's image", "content byte"])
def test_no_byte_of_a_bad_block_reaches_the_output(gpu, oracle, ref, case):
    w = written(gpu, oracle, ref, "by-tag", CONFIGS[1])
    files = files_of(w["tree"])
    offsets, total = Restore.layout(w["vi"], 64)
    si = parse_store_index(w["si"])
    images, bad, flag = damaged_case(w, case)
    c0, n = int(si["block_offsets"][bad]), int(si["block_counts"][bad])
    bad_hashes = set(int(h) for h in si["chunk_hashes"][c0 : c0 + n])
    fed = [(at, size) for h, at, size in occurrences(w["vi"], offsets) if h in bad_hashes]
    assert fed
    code, res, out, rs = restore(gpu, w["vi"], w["si"], images, offsets, total, verify=True)
    assert code == errno.EBADF
    status = rs.block_status(si["block_hashes"])
    assert status[bad] == flag and (np.delete(status, bad) == 0).all(), (case, status[bad])
    assert res.blocks_bad == 1 and res.chunks_mismatched == (1 if case == "content byte" else 0)
    want = expected_output(files, offsets, total)
    for at, size in fed:
        want[at : at + size] = FILL
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])
    assert res.occurrences_written == res.occurrences - len(fed) and res.bytes_written == sum(len(f) for f in files) - sum(s for _, s in fed)
    if case != "content byte":
        return
    # ---- without verify the flipped byte goes through: finish 0, and the output differs in exactly its occurrences ----
    code, res, out, rs = restore(gpu, w["vi"], w["si"], images, offsets, total, verify=False)
    assert code == 0 and res.blocks_bad == 0 and (rs.block_status(si["block_hashes"]) == 0).all()
    want = expected_output(files, offsets, total)
    sizes = si["chunk_sizes"][c0 : c0 + n].astype(np.int64)
    k = int(np.searchsorted(np.cumsum(sizes), 5, side="right"))  # the chunk that holds byte 5 of the block
    rel = 5 - int(sizes[:k].sum())
    hit = [at + rel for h, at, size in occurrences(w["vi"], offsets) if h == int(si["chunk_hashes"][c0 + k])]
    assert hit and np.flatnonzero(out != want).tolist() == sorted(hit)
    assert all(int(out[p]) == int(want[p]) ^ 0x01 for p in hit)


# ---- 7. refusals ----


def test_refusals_leave_the_context_and_the_session_usable(gpu, oracle, ref):
    w = written(gpu, oracle, ref, "by-tag", CONFIGS[1])
    files = files_of(w["tree"])
    offsets, total = Restore.layout(w["vi"], 64)
    si = parse_store_index(w["si"])
    hashes, images = si["block_hashes"], w["images"]

    def refused(code, fn):
        with pytest.raises(LongtailHipError) as e:
            fn()
        assert e.value.code == code, (e.value.code, code)

    # ---- from create ----
    end = max(int(o) + len(f) for o, f in zip(offsets, files) if len(f))
    refused(errno.EINVAL, lambda: Restore(gpu, w["vi"], w["si"], offsets, end - 1))  # the last window passes out_bytes
    refused(errno.ENOENT, lambda: Restore(gpu, w["vi"], without_last_block(w["si"]), offsets, total))
    other_id = np.frombuffer(w["si"], np.uint8).copy()
    other_id[4:8] = np.array([BLK2], np.uint32).view(np.uint8)
    refused(errno.EINVAL, lambda: Restore(gpu, w["vi"], other_id.tobytes(), offsets, total))
    refused(errno.EBADF, lambda: Restore(gpu, w["vi"][:-1], w["si"], offsets, total))
    refused(errno.EBADF, lambda: Restore(gpu, w["vi"], w["si"][:-1], offsets, total))
    refused(errno.EBADF, lambda: Restore(gpu, w["vi"][:20], w["si"][:12], offsets, total))
    # ---- from blocks: nothing is queued, nothing changes ----
    rs = keep(Restore(gpu, w["vi"], w["si"], offsets, total, verify=True))
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    tagged = int(np.flatnonzero(si["block_tags"] != 0)[0])
    refused(errno.ENOENT, lambda: deliver(rs, np.array([int(hashes[0]) ^ 1], np.uint64), [images[0]], out))
    refused(errno.EEXIST, lambda: deliver(rs, hashes[[1, 2, 1]], [images[1], images[2], images[1]], out))
    assert rs.scratch_bound(hashes[[tagged]]) > 0
    refused(errno.ENOMEM, lambda: deliver(rs, hashes[[tagged]], [images[tagged]], out, scratch_extra=-1))
    deliver(rs, hashes[[tagged]], [images[tagged]], out)
    refused(errno.EEXIST, lambda: deliver(rs, hashes[[0, tagged]], [images[0], images[tagged]], out))  # delivered before
    gpu.sync()
    rest = [b for b in range(len(images)) if b != tagged]
    deliver(rs, hashes[rest], [images[b] for b in rest], out)
    code, res = rs.finish()
    assert code == 0 and res.blocks_delivered == len(images)
    want = expected_output(files, offsets, total)
    got = out.cpu().numpy()
    assert (got == want).all(), int(np.flatnonzero(got != want)[0])
    # ---- and a full round trip on the same context ----
    check_round_trip(gpu, w)


# ---- 8. lthip_seen_find ----


def test_seen_find_is_the_first_position_or_absent(gpu):
    rng = np.random.default_rng(12)
    distinct = rng.integers(1, 2**63, 30_000).astype(np.uint64)
    hashes = distinct[rng.integers(0, len(distinct), 50_000)]
    hashes[777] = np.uint64(0xFFFFFFFFFFFFFFFF)  # the table's empty key
    seen = keep(Seen(gpu, 0))
    for a, b in ((0, 400), (400, 20_000), (20_000, 50_000)):
        seen.add(dev_u64(hashes[a:b]))
    assert seen.grown >= 2 and seen.total == len(hashes)
    first = {}
    for i, h in enumerate(hashes.tolist()):
        first.setdefault(h, i)
    absent = np.setdiff1d(rng.integers(1, 2**63, 1_100).astype(np.uint64), hashes)[:1000]
    assert len(absent) == 1000
    ask = np.concatenate([hashes, absent])
    got = seen.find(dev_u64(ask)).cpu().numpy().view(np.uint32)
    want = np.array([first.get(h, 0xFFFFFFFF) for h in ask.tolist()], np.uint32)
    assert (got == want).all(), int(np.flatnonzero(got != want)[0])
    fresh = keep(Seen(gpu, 0))  # a table that never saw the empty key's hash
    got = fresh.find(dev_u64(np.array([0xFFFFFFFFFFFFFFFF, 5], np.uint64))).cpu().numpy().view(np.uint32)
    assert (got == 0xFFFFFFFF).all()
