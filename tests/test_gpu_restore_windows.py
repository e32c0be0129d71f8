"""-m gpu: byte windows of assets (lthip_restore_create_windows, include/longtail_hip.h "byte windows of assets").

  1 a clip sweep on a version built by hand: every chunk length of a list with every (skip, clip) of two lists at cycling destination
    residues, windows over two and three chunks on and off chunk boundaries, with verify and without
  2 whole-asset windows are lthip_restore_create: output, needed blocks and every field of the result
  3 needed_blocks shrinks to the blocks a window touches; the others are accepted, counted and cost no scratch
  4 a StoreIndex without the chunks no window touches is accepted, ENOENT when one does
  5 round trips of what the stream session wrote: 64 random windows per store, in one batch and in three
  6 THE GUARANTEE: a bad chunk that no window overlaps still takes its whole block out
  7 refusals, one at a time; zero-length windows; carry on a window session
  8 a rank's share: lthip_restore_rank_windows per rank, the files put together again from the ranks' buffers

In every test the output buffer is filled with 0xA5 first and compared WHOLE with what is expected.  Every comparison is equality."""
import ctypes as C
import errno

import numpy as np
import pytest
import torch

from longtail_amd.dist import JobPartition
from longtail_amd.lib import (RESTORE_BAD_CHUNK, RESTORE_BAD_HEADER, LongtailHipError, Restore, RestoreConfig, restore_asset_sizes,
                              restore_rank_windows)
from tests.restore_util import (BLK2, BLK3, MEOW, build_store_index, build_version_index, parse_store_index, parse_version_index, raw_image,
                                without_last_block)
from tests.restore_windows_util import (FILL, LENGTHS, SHARE_NAMES, SHARE_SIZES, SWEEP_ASSETS, SWEEP_BLOCKS, expected_windows_output,
                                        model_occurrences, place, share_tree, sweep_chunks, sweep_files, sweep_version, sweep_windows)
from tests.test_gpu_ingest_by_tag import CONFIGS
from tests.test_gpu_ingest_stream import _sessions
from tests.test_gpu_restore import _open, deliver, expected_output, files_of, keep, restore, written
from tests.test_restore_windows_san import invalid_windows, raw_table

pytestmark = pytest.mark.gpu
_made = {}


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    yield
    while _open:
        _open.pop().close()
    while _sessions:
        _sessions.pop().close()


def restore_windows(gpu, vi, si, images_by_hash, windows, out_bytes, verify=True, batches=1, extra=()):
    """A window session fed its needed blocks (and the blocks `extra`) in `batches` calls -> (finish's code, result, output, session)."""
    rs = keep(Restore(gpu, vi, si, None, out_bytes, verify=verify, windows=windows))
    out = torch.full((max(out_bytes, 1),), FILL, dtype=torch.uint8, device="cuda")
    hashes = np.concatenate([rs.needed_blocks(), np.asarray(extra, np.uint64)]).astype(np.uint64)
    for k in range(batches):
        mine = hashes[k::batches]
        if len(mine):
            deliver(rs, mine, [images_by_hash[int(h)] for h in mine], out)
    code, res = rs.finish()
    return code, res, out.cpu().numpy()[:out_bytes], rs


def same(got, want):
    assert (got == want).all(), int(np.flatnonzero(got != want)[0])


def sweep(oracle):
    """The sweep's version with real chunk hashes: dict(vi, si, files, images (by block hash), block_hashes, hashes)."""
    if "sweep" not in _made:
        chunks = sweep_chunks()
        content = np.concatenate(chunks)
        starts = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])
        hashes = oracle.blake3_many(content, starts, LENGTHS)
        lens = np.array(LENGTHS, np.uint32)
        block_hashes = [oracle.blake3(np.frombuffer(hashes[cs].tobytes(), np.uint8)) for cs in SWEEP_BLOCKS]
        vi, si = sweep_version(hashes, block_hashes)
        images = {int(h): raw_image(h, BLK3, hashes[cs], lens[cs], np.concatenate([chunks[c] for c in cs]))
                  for h, cs in zip(block_hashes, SWEEP_BLOCKS)}
        _made["sweep"] = dict(vi=vi, si=si, files=sweep_files(chunks), images=images, block_hashes=np.array(block_hashes, np.uint64), hashes=hashes)
    return _made["sweep"]


def chunk_span(asset, position):
    """Where the chunk at `position` of a sweep asset lies in it -> (first byte, length)."""
    cs = SWEEP_ASSETS[asset]
    return sum(LENGTHS[c] for c in cs[:position]), LENGTHS[cs[position]]


# ---- 1. the clip sweep ----


@pytest.mark.parametrize("verify", [True, False])
def test_every_skip_and_clip_at_every_alignment(gpu, oracle, verify):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    occ, selected = model_occurrences(s["vi"], windows)
    assert {d % 16 for *_, d in occ} == set(range(16)) and selected == 3
    code, res, out, rs = restore_windows(gpu, s["vi"], s["si"], s["images"], windows, out_bytes, verify=verify)
    assert code == 0
    same(out, expected_windows_output(s["files"], windows, out_bytes))
    assert res.occurrences == res.occurrences_written == len(occ) and res.bytes_written == sum(c for _, _, _, c, _ in occ)
    assert res.bytes_written == sum(n for _, _, n, _ in windows)
    assert (res.assets_selected, res.blocks_needed, res.blocks_delivered, res.blocks_bad, res.chunks_mismatched) == (3, 3, 3, 0, 0)
    assert (rs.needed_blocks() == s["block_hashes"]).all()


# ---- 2. whole-asset windows are lthip_restore_create ----

RESULT_FIELDS = ["assets_selected", "occurrences", "occurrences_written", "bytes_written", "blocks_needed", "blocks_delivered", "blocks_unneeded",
                 "blocks_bad", "chunks_mismatched", "decoded_bytes", "base_occurrences", "base_bytes", "base_chunks_mismatched"]


@pytest.mark.parametrize("which", ["every asset", "every second asset"])
def test_whole_asset_windows_equal_the_ordinary_session(gpu, oracle, ref, which):
    w = written(gpu, oracle, ref, "by-tag", CONFIGS[0])
    files = files_of(w["tree"])
    offsets, total = Restore.layout(w["vi"], 64)
    if which == "every second asset":
        offsets = np.array([int(o) if a % 2 == 0 else Restore.SKIP for a, o in enumerate(offsets)], np.uint64)
    hashes = parse_store_index(w["si"])["block_hashes"]
    images = {int(h): i for h, i in zip(hashes, w["images"])}
    plain = keep(Restore(gpu, w["vi"], w["si"], offsets, total, verify=True))
    needed = plain.needed_blocks()
    out = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    deliver(plain, needed, [images[int(h)] for h in needed], out)
    code, want_res = plain.finish()
    assert code == 0
    want = out.cpu().numpy()
    same(want, expected_output(files, offsets, total))
    assert any(len(f) == 0 for f in files), "a directory or an empty file among the windows"
    windows = [(a, 0, len(f), int(o)) for a, (f, o) in enumerate(zip(files, offsets)) if int(o) != Restore.SKIP]
    code, res, got, rs = restore_windows(gpu, w["vi"], w["si"], images, windows, total)
    assert code == 0
    same(got, want)
    assert (rs.needed_blocks() == needed).all() and len(needed) == res.blocks_needed
    assert [getattr(res, f) for f in RESULT_FIELDS] == [getattr(want_res, f) for f in RESULT_FIELDS]
    assert res.assets_selected == len(windows) and res.bytes_written == sum(n for _, _, n, _ in windows)


# ---- 3. needed_blocks shrinks ----


def test_only_the_blocks_a_window_touches_are_needed(gpu, oracle):
    s = sweep(oracle)
    # chunks 3 and 4 are block 1's: pieces of them at every position they have in the three assets
    spans = []
    for a, cs in enumerate(SWEEP_ASSETS):
        for k, c in enumerate(cs):
            if c in SWEEP_BLOCKS[1]:
                begin, n = chunk_span(a, k)
                spans += [(a, begin + 1, n - 2), (a, begin, n)]
    windows, out_bytes = place(spans)
    rs = keep(Restore(gpu, s["vi"], s["si"], None, out_bytes, windows=windows))
    assert rs.needed_blocks().tolist() == [int(s["block_hashes"][1])]
    others = s["block_hashes"][[0, 2]]
    assert rs.scratch_bound(others) == 0 and rs.scratch_bound(s["block_hashes"]) == 0
    code, res, out, rs = restore_windows(gpu, s["vi"], s["si"], s["images"], windows, out_bytes, extra=others)
    assert code == 0 and (res.blocks_needed, res.blocks_delivered, res.blocks_unneeded, res.blocks_bad) == (1, 3, 2, 0)
    same(out, expected_windows_output(s["files"], windows, out_bytes))
    assert (rs.block_status(s["block_hashes"]) == 0).all()


def test_a_tagged_block_no_window_touches_costs_no_scratch(gpu, oracle, ref):
    w = written(gpu, oracle, ref, "lz4", CONFIGS[1])
    files = files_of(w["tree"])
    si = parse_store_index(w["si"])
    images = {int(h): i for h, i in zip(si["block_hashes"], w["images"])}
    a = int(np.argmax([len(f) for f in files]))
    windows = [(a, len(files[a]) // 2, 1, 5)]
    rs = keep(Restore(gpu, w["vi"], w["si"], None, 64, windows=windows))
    needed = rs.needed_blocks()
    assert len(needed) == 1 < len(si["block_hashes"])
    tag_of = {int(h): int(t) for h, t in zip(si["block_hashes"], si["block_tags"])}
    assert any(tag_of.values())
    other = np.array([h for h in si["block_hashes"] if h != needed[0] and tag_of[int(h)]][:1], np.uint64)
    assert len(other) == 1 and rs.scratch_bound(other) == 0, "a tagged block no window touches"
    assert (rs.scratch_bound(needed) > 0) == (tag_of[int(needed[0])] != 0)
    code, res, out, _ = restore_windows(gpu, w["vi"], w["si"], images, windows, 64, extra=other)
    assert code == 0 and (res.blocks_needed, res.blocks_delivered, res.blocks_unneeded, res.bytes_written, res.occurrences) == (1, 2, 1, 1, 1)
    same(out, expected_windows_output(files, windows, 64))


# ---- 4. a partial StoreIndex ----


def test_a_store_index_without_untouched_chunks_is_accepted(gpu, oracle):
    s = sweep(oracle)
    partial = without_last_block(s["si"])  # chunks 5 and 6 are gone
    spans, over = [], []
    for a, cs in enumerate(SWEEP_ASSETS):
        for k, c in enumerate(cs):
            begin, n = chunk_span(a, k)
            (over if c in SWEEP_BLOCKS[2] else spans).append((a, begin, n))
    # ... and windows that end on the last byte before a missing chunk, and start on the first byte behind one
    begin, n = chunk_span(0, 5)
    spans += [(0, begin - 40, 40), (1, LENGTHS[6] + LENGTHS[5], 20)]
    windows, out_bytes = place(spans)
    code, res, out, rs = restore_windows(gpu, s["vi"], partial, s["images"], windows, out_bytes)
    assert code == 0 and res.blocks_needed == 2 and (rs.needed_blocks() == s["block_hashes"][:2]).all()
    same(out, expected_windows_output(s["files"], windows, out_bytes))
    for a, off, n in (over[0], (0, begin - 1, 2), (1, LENGTHS[6] + LENGTHS[5] - 1, 2)):  # whole, by its first byte, by its last byte
        with pytest.raises(LongtailHipError) as e:
            Restore(gpu, s["vi"], partial, None, out_bytes, windows=windows + [(a, off, n, 0)])
        assert e.value.code == errno.ENOENT
    code, res, out, _ = restore_windows(gpu, s["vi"], partial, s["images"], windows, out_bytes, verify=False)
    assert code == 0
    same(out, expected_windows_output(s["files"], windows, out_bytes))


# ---- 5. round trips of what the stream session wrote ----

ROUND_TRIPS = [(codec, CONFIGS[1], BLK3) for codec in ("none", "lz4", "zstd", "by-tag")] + [("lz4", CONFIGS[1], BLK2), ("zstd", CONFIGS[1], MEOW)]


def random_windows(files, seed, count=64):
    rng = np.random.default_rng(seed)
    full = [a for a, f in enumerate(files) if len(f)]
    spans = []
    for i in range(count - 2):
        a = int(rng.choice(full))
        size = len(files[a])
        n = 1 if i % 8 == 0 else int(rng.integers(1, min(size, 50_000) + 1))
        off = size - n if i % 8 == 1 else int(rng.integers(0, size - n + 1))  # (i % 8 == 1: the window ends at the asset's last byte)
        spans.append((a, off, n))
    spans += [spans[5], spans[9]]  # the same bytes twice, at other destinations
    return place(spans)


@pytest.mark.parametrize("codec,cfg,hash_id", ROUND_TRIPS)
def test_random_windows_of_the_sessions_own_stores(gpu, oracle, ref, codec, cfg, hash_id):
    w = written(gpu, oracle, ref, codec, cfg, hash_id)
    files = files_of(w["tree"])
    hashes = parse_store_index(w["si"])["block_hashes"]
    images = {int(h): i for h, i in zip(hashes, w["images"])}
    windows, out_bytes = random_windows(files, 77)
    assert sum(n == 1 for _, _, n, _ in windows) >= 8 and sum(off + n == len(files[a]) for a, off, n, _ in windows) >= 8
    want = expected_windows_output(files, windows, out_bytes)
    occ, selected = model_occurrences(w["vi"], windows)
    for batches in (1, 3):
        code, res, out, rs = restore_windows(gpu, w["vi"], w["si"], images, windows, out_bytes, batches=batches)
        assert code == 0
        same(out, want)
        assert res.occurrences == res.occurrences_written == len(occ) and res.bytes_written == sum(n for _, _, n, _ in windows)
        assert res.assets_selected == selected and res.blocks_needed == res.blocks_delivered == len(rs.needed_blocks()) and res.blocks_bad == 0
        need = {h for h, *_ in occ}
        si = parse_store_index(w["si"])
        holds = [b for b in range(len(hashes)) if need & set(int(x) for x in si["chunk_hashes"][int(si["block_offsets"][b]):][: int(si["block_counts"][b])])]
        assert rs.needed_blocks().tolist() == [int(hashes[b]) for b in holds]


# ---- 6. THE GUARANTEE ----


def guarantee_windows():
    """Pieces of chunk 5 (block 2) and of chunks 1 and 3 (blocks 0 and 1); nothing overlaps chunk 6, block 2's other chunk."""
    spans, fed_by_2 = [], []
    for a, cs in enumerate(SWEEP_ASSETS):
        for k, c in enumerate(cs):
            begin, n = chunk_span(a, k)
            if c == 5:
                fed_by_2 += [len(spans), len(spans) + 1]
                spans += [(a, begin + 3, 100), (a, begin, n)]
            elif c in (1, 3):
                spans.append((a, begin + 1, n - 1))
    windows, out_bytes = place(spans)
    return windows, out_bytes, fed_by_2


def test_a_bad_chunk_outside_every_window_takes_its_block_out(gpu, oracle):
    s = sweep(oracle)
    windows, out_bytes, fed = guarantee_windows()
    bad = int(s["block_hashes"][2])
    images = dict(s["images"])
    images[bad] = images[bad].copy()
    images[bad][20 + 12 * 2 + LENGTHS[5] + 1000] ^= 0x40  # a payload byte of chunk 6
    want = expected_windows_output(s["files"], windows, out_bytes)
    code, res, out, rs = restore_windows(gpu, s["vi"], s["si"], images, windows, out_bytes, verify=False)
    assert code == 0 and res.blocks_bad == 0  # without verify the windows are restored: the flipped byte lies in none
    same(out, want)
    code, res, out, rs = restore_windows(gpu, s["vi"], s["si"], images, windows, out_bytes, verify=True)
    assert code == errno.EBADF
    assert rs.block_status(s["block_hashes"]).tolist() == [0, 0, RESTORE_BAD_CHUNK]
    assert (res.blocks_bad, res.chunks_mismatched, res.blocks_needed, res.blocks_delivered) == (1, 1, 3, 3)
    kept = want.copy()
    for i in fed:
        kept[windows[i][3] : windows[i][3] + windows[i][2]] = FILL
    same(out, kept)
    assert res.occurrences_written == res.occurrences - len(fed) and res.bytes_written == sum(n for k, (_, _, n, _) in enumerate(windows) if k not in fed)


@pytest.mark.parametrize("verify", [True, False])
def test_nothing_of_a_block_with_a_damaged_header_reaches_the_output(gpu, oracle, verify):
    s = sweep(oracle)
    windows, out_bytes, fed = guarantee_windows()
    bad = int(s["block_hashes"][2])
    images = dict(s["images"])
    images[bad] = images[bad].copy()
    images[bad][20 + 8 + 2] ^= 0x04  # the recorded hash of chunk 6, which no window overlaps
    code, res, out, rs = restore_windows(gpu, s["vi"], s["si"], images, windows, out_bytes, verify=verify)
    assert code == errno.EBADF and rs.block_status(s["block_hashes"]).tolist() == [0, 0, RESTORE_BAD_HEADER]
    kept = expected_windows_output(s["files"], windows, out_bytes)
    for i in fed:
        kept[windows[i][3] : windows[i][3] + windows[i][2]] = FILL
    same(out, kept)
    assert res.blocks_bad == 1 and res.chunks_mismatched == 0


# ---- 7. refusals ----


def share(oracle):
    """The rank-share tree with real chunk hashes, three raw blocks: dict(vi, si, files, images, block_hashes)."""
    if "share" not in _made:
        files, chunks, asset_chunks, lens, blocks = share_tree()
        content = np.concatenate(chunks)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
        hashes = oracle.blake3_many(content, starts, lens)
        lens = np.array(lens, np.uint32)
        block_hashes = [oracle.blake3(np.frombuffer(hashes[cs].tobytes(), np.uint8)) for cs in blocks]
        vi = build_version_index(BLK3, 1, SHARE_NAMES, asset_chunks, hashes, lens)
        si = build_store_index(BLK3, [(int(h), 0, cs) for h, cs in zip(block_hashes, blocks)], hashes, lens)
        images = {int(h): raw_image(h, BLK3, hashes[cs], lens[cs], np.concatenate([chunks[c] for c in cs])) for h, cs in zip(block_hashes, blocks)}
        _made["share"] = dict(vi=vi, si=si, files=files, images=images, block_hashes=np.array(block_hashes, np.uint64))
    return _made["share"]


def create_raw(gpu, vi, si, table, count, out_bytes):
    """lthip_restore_create_windows on a raw table (None: a NULL pointer) -> the error code; a session that was made is destroyed."""
    a, b = np.frombuffer(vi, np.uint8), np.frombuffer(si, np.uint8)
    cfg = RestoreConfig(C.sizeof(RestoreConfig), 1)
    h = C.c_void_p(0x5555)
    err = gpu.lib.dll.lthip_restore_create_windows(gpu.h, C.byref(cfg), a.ctypes.data, len(a), b.ctypes.data, len(b), count,
                                                   None if table is None else table.ctypes.data, out_bytes, C.byref(h))
    if err == 0:
        gpu.lib.dll.lthip_restore_destroy(h)
    else:
        assert not h.value, "a refused create hands out no session"
    return err


def test_refusals_one_at_a_time_and_a_good_session_afterwards(gpu, oracle):
    s = sweep(oracle)
    windows, out_bytes = sweep_windows()
    good = raw_table([(a, 0, off, n, dst) for a, off, n, dst in windows[:5]])
    assert create_raw(gpu, s["vi"], s["si"], good, len(good), out_bytes) == 0
    for bad in invalid_windows(out_bytes):
        table = raw_table([(a, 0, off, n, dst) for a, off, n, dst in windows[:5]] + [bad])
        assert create_raw(gpu, s["vi"], s["si"], table, len(table), out_bytes) == errno.EINVAL, bad
        assert create_raw(gpu, s["vi"], s["si"], table, len(table) - 1, out_bytes) == 0
    assert create_raw(gpu, s["vi"], s["si"], None, 1, out_bytes) == errno.EINVAL
    assert create_raw(gpu, s["vi"], s["si"], None, 0, out_bytes) == 0
    # 32 768 windows over an asset of 65 536 one-byte chunks: 2^31 occurrences, refused before anything of that size is allocated
    n = 65536
    big = build_version_index(BLK3, 32768, ["big"], [list(range(n))], np.arange(1, n + 1, dtype=np.uint64), np.ones(n, np.uint32))
    many = raw_table([(0, 0, 0, n, 0)] * 32768)
    assert create_raw(gpu, big, s["si"], many, len(many), n) == errno.EINVAL
    # what lthip_restore_create refuses: malformed blobs, other hash identifiers
    assert create_raw(gpu, s["vi"][:-1], s["si"], good, len(good), out_bytes) == errno.EBADF
    assert create_raw(gpu, s["vi"], s["si"][:-1], good, len(good), out_bytes) == errno.EBADF
    other_id = np.frombuffer(s["si"], np.uint8).copy()
    other_id[4:8] = np.array([BLK2], np.uint32).view(np.uint8)
    assert create_raw(gpu, s["vi"], other_id.tobytes(), good, len(good), out_bytes) == errno.EINVAL
    gpu.sync()
    code, res, out, _ = restore_windows(gpu, s["vi"], s["si"], s["images"], windows, out_bytes)
    assert code == 0
    same(out, expected_windows_output(s["files"], windows, out_bytes))


def test_zero_length_windows_plan_nothing_and_a_window_session_has_no_base(gpu, oracle):
    t = share(oracle)
    empty, directory = SHARE_NAMES.index("empty"), SHARE_NAMES.index("dir/")
    windows = [(empty, 0, 0, 0), (directory, 0, 0, 64), (empty, 0, 0, 7)]
    code, res, out, rs = restore_windows(gpu, t["vi"], t["si"], t["images"], windows, 64)
    assert code == 0 and len(rs.needed_blocks()) == 0
    assert (res.assets_selected, res.occurrences, res.bytes_written, res.blocks_needed) == (2, 0, 0, 0)
    same(out, np.full(64, FILL, np.uint8))
    for a in (empty, directory):  # a byte of an asset that has none
        with pytest.raises(LongtailHipError) as e:
            Restore(gpu, t["vi"], t["si"], None, 64, windows=[(a, 0, 1, 0)])
        assert e.value.code == errno.EINVAL
    five = SHARE_NAMES.index("five")
    rs = keep(Restore(gpu, t["vi"], t["si"], None, 64, windows=[(five, 10, 0, 3), (five, 4999, 1, 9)]))
    buf = torch.full((64,), FILL, dtype=torch.uint8, device="cuda")
    for call in (lambda: rs.carry(buf, buf), lambda: rs.carry_in_place(buf, None)):
        with pytest.raises(LongtailHipError) as e:
            call()
        assert e.value.code == errno.EINVAL
    assert rs.in_place_scratch_bound() == 0 and rs.in_place_stats() == (0, 0, 0, 0)
    needed = rs.needed_blocks()
    deliver(rs, needed, [t["images"][int(h)] for h in needed], buf)
    code, res = rs.finish()
    assert code == 0 and (res.assets_selected, res.occurrences, res.bytes_written) == (1, 1, 1)
    want = np.full(64, FILL, np.uint8)
    want[9] = t["files"][five][4999]
    same(buf.cpu().numpy(), want)


# ---- 8. a rank's share ----


@pytest.mark.parametrize("align", [1, 64])
@pytest.mark.parametrize("policy", ["range", "lpt", "mod"])
@pytest.mark.parametrize("world", [2, 3])
def test_the_ranks_shares_put_the_files_together_again(gpu, oracle, world, policy, align):
    t = share(oracle)
    sizes, target = restore_asset_sizes(t["vi"])
    assert sizes.tolist() == SHARE_SIZES and target == 1
    part = JobPartition(sizes, target, world, policy)
    assert part.job_count == sum(1 + n // 1024 for n in SHARE_SIZES) > 10
    rebuilt = [np.full(n, 0, np.uint8) for n in SHARE_SIZES]
    covered = [np.zeros(n, np.int64) for n in SHARE_SIZES]
    needed = set()
    for rank in range(world):
        rows, total = restore_rank_windows(part.job_asset, part.job_offset, part.job_size, part.job_rank, rank, align)
        windows = [tuple(int(x) for x in r) for r in rows]
        assert sum(n for _, _, n, _ in windows) == int(part.rank_bytes[rank]) and all(d % align == 0 for *_, d in windows)
        code, res, out, rs = restore_windows(gpu, t["vi"], t["si"], t["images"], windows, total)
        assert code == 0 and res.bytes_written == int(part.rank_bytes[rank])
        same(out, expected_windows_output(t["files"], windows, total))
        needed |= set(rs.needed_blocks().tolist())
        for a, off, n, dst in windows:
            rebuilt[a][off : off + n] = out[dst : dst + n]
            covered[a][off : off + n] += 1
    for a, f in enumerate(t["files"]):
        assert (covered[a] == 1).all(), SHARE_NAMES[a]
        same(rebuilt[a], f)
    offsets, total = Restore.layout(t["vi"], 1)
    code, res, out, rs = restore(gpu, t["vi"], t["si"], [t["images"][int(h)] for h in t["block_hashes"]], offsets, total)
    assert code == 0 and needed == set(rs.needed_blocks().tolist()) and len(needed) == 3
    same(out, expected_output(t["files"], offsets, total))
