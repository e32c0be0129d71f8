"""-m gpu: a base for the restore session (lthip_restore_create_from_base, lthip_restore_carry; include/longtail_hip.h, "updating a
resident version") -- version N lies restored in device memory, version N + 1 takes the chunks the two share from there.

  1. a run and alignment sweep on versions built by hand: runs of 1, 63, 64, 65 and 300 entries, a run over entry 256 of the list, one of
     more than 200 KiB, chunks of 1, 15, 16, 17 and 4097 bytes, every destination residue mod 16 against every source residue mod 4,
     base-fed between store-fed chunks and the reverse, a chunk that ends at the last byte of the base, one base chunk feeding many
     occurrences, a chunk the base holds with another size; 'blk3', 'blk2' and 'meow', verify off and on
  2. version A -> version B of tests/test_gpu_ingest_store.py, B's StoreIndex the one the stream session wrote against a store that holds A
  3. the base wins: B's full StoreIndex plus the base needs only the blocks with a chunk no resident asset has
  4. a partial base (every second asset resident) and a partial target (version_diff's added + content-modified assets)
  5. a damaged base: with verify the chunk's occurrences keep what the output held, without it the base is trusted
  6. carry before, between and after the blocks calls; refusals leave the session and the context usable

In every test the output buffer is filled with 0xA5 first and compared WHOLE with what is expected.  Every comparison is equality."""
import ctypes as C
import errno

import numpy as np
import pytest
import torch

from longtail_amd.lib import LongtailHipError, Restore, RestoreBase, RestoreConfig, Store, version_diff
from tests import test_gpu_ingest_store as store_tests
from tests.restore_util import BLK2, BLK3, MEOW, build_store_index, parse_store_index, parse_version_index, raw_image
from tests.test_gpu_ingest_store import STORE_CONFIGS, next_version, tag_of
from tests.test_gpu_ingest_stream import _sessions, slices_of, tree_of
from tests.test_gpu_restore import FILL, deliver, expected_output, files_of, occurrences
from tests.update_util import asset_fields, build_version_index

pytestmark = pytest.mark.gpu

_open, _runs = [], {}


@pytest.fixture(autouse=True)
def _objects_end_with_their_test():
    yield
    for held in (_open, store_tests._open, _sessions):
        while held:
            held.pop().close()


def keep(obj):
    _open.append(obj)
    return obj


def refused(code, fn):
    with pytest.raises(LongtailHipError) as e:
        fn()
    assert e.value.code == code, (e.value.code, code)


def first_places(vi, offsets):
    """What a base holds: chunk hash -> (offset of its first occurrence in a resident asset, size)."""
    places = {}
    for h, at, n in occurrences(vi, offsets):
        places.setdefault(h, (at, n))
    return places


def fed_by(places, occ):
    """The occurrences (hash, destination, length) the base feeds: it holds the hash with the same size."""
    return [o for o in occ if o[0] in places and places[o[0]][1] == o[2]]


def blocks_with_a_chunk_outside(si, places, occ):
    """The hashes of the StoreIndex's blocks that hold a chunk some occurrence needs and the base does not feed, in StoreIndex order."""
    p = parse_store_index(si)
    wanted = {o[0] for o in occ} - {o[0] for o in fed_by(places, occ)}
    out = []
    for b, h in enumerate(p["block_hashes"]):
        c0, n = int(p["block_offsets"][b]), int(p["block_counts"][b])
        if wanted & set(p["chunk_hashes"][c0 : c0 + n].tolist()):
            out.append(int(h))
    return out


def update(gpu, target, store, base, out_bytes, verify=True, carry_at=1, blocks=None, pad=0):
    """target = (vi, asset offsets), store = (si, images in StoreIndex order), base = (vi, asset offsets, base bytes, device tensor).  The
    needed blocks (or `blocks`: hashes) are delivered in two calls, carry comes before call `carry_at`.
    -> (finish's code, the result, the output, the needed blocks)"""
    index_of = {int(h): b for b, h in enumerate(parse_store_index(store[0])["block_hashes"])}
    rs = keep(Restore(gpu, target[0], store[0], target[1], out_bytes, verify=verify, base=base[:3]))
    needed = [int(h) for h in rs.needed_blocks()]
    todo = needed if blocks is None else blocks
    out = torch.full((max(out_bytes + pad, 1),), FILL, dtype=torch.uint8, device="cuda")
    calls = [todo[: len(todo) // 2], todo[len(todo) // 2 :]]
    for k in range(3):
        if k == carry_at:
            rs.carry(base[3], out)
        if k < 2 and calls[k]:
            deliver(rs, np.array(calls[k], np.uint64), [store[1][index_of[h]] for h in calls[k]], out)
    code, res = rs.finish()
    return code, res, out.cpu().numpy(), needed


# ---- 1. the run and alignment sweep ----


def device_hashes(gpu, hash_id, chunks):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in chunks])[:-1]]).astype(np.int64)
    dev = torch.from_numpy(np.concatenate(chunks)).cuda()
    fn = {BLK3: gpu.hash_ranges, BLK2: gpu.blake2s_ranges, MEOW: gpu.meow_ranges}[hash_id]
    got = fn(dev, torch.from_numpy(offs).cuda(), torch.tensor([len(c) for c in chunks], dtype=torch.int32, device="cuda"))
    return got.cpu().numpy().view(np.uint64).copy()


def version_of(hash_id, names, asset_chunks, hashes, sizes):
    """A VersionIndex over the ids of a shared chunk pool: its own unique list holds the chunks it uses, in order of first use."""
    local = {}
    for cs in asset_chunks:
        for c in cs:
            local.setdefault(c, len(local))
    ids = list(local)
    return build_version_index(hash_id, 32768, names, [[local[c] for c in cs] for cs in asset_chunks], [hashes[c] for c in ids],
                               [sizes[c] for c in ids])


def sweep_case(gpu, hash_id):
    rng = np.random.default_rng(21)
    pool = []

    def new(n):
        pool.append(rng.integers(0, 256, int(n)).astype(np.uint8))
        return len(pool) - 1

    g = [new(n) for n in rng.integers(18, 31, 500)]       # the long lists of small chunks
    small = [new(n) for n in (1, 15, 16, 17, 4097, 2, 3, 33)]
    big = [new(n) for n in (60000, 50001, 65536, 40000)]  # one run of more than 200 KiB
    s = [new(n) for n in rng.integers(5, 40, 12)]         # the store's alone
    z, w = new(700), new(900)                             # the base holds z's hash with another size, and w in an asset that is not resident
    hashes = device_hashes(gpu, hash_id, pool)
    assert len(set(hashes.tolist())) == len(pool)
    sizes = [len(c) for c in pool]
    # ---- the base: assets at odd offsets, the last one ends at the last byte of the buffer ----
    base_names = ["base/g", "base/small", "base/absent", "base/z", "base/big"]
    base_chunks = [g, small, [w], [z], big]
    base_sizes = list(sizes)
    base_sizes[z] = sizes[z] + 3
    z_in_base = rng.integers(0, 256, base_sizes[z]).astype(np.uint8)
    base_offsets, at = [], 3
    for name, cs in zip(base_names, base_chunks):
        base_offsets.append(Restore.SKIP if name == "base/absent" else at)
        if name != "base/absent":
            at += sum(base_sizes[c] for c in cs) + 5
    base_bytes = at - 5
    base_host = np.full(base_bytes, 0x11, np.uint8)
    for off, cs in zip(base_offsets, base_chunks):
        if off != Restore.SKIP:
            data = np.concatenate([z_in_base if c == z else pool[c] for c in cs])
            base_host[off : off + len(data)] = data
    assert base_offsets[-1] + sum(sizes[c] for c in big) == base_bytes, "a chunk ends at the last byte of the base"
    base_vi = version_of(hash_id, base_names, base_chunks, hashes, base_sizes)
    # ---- the target ----
    names = ["t/runs", "t/singles", "t/store", "t/big", "t/store_first", "t/empty"]
    chunks = [[g[0], s[0]] + g[1:64] + [s[1]] + g[64:128] + [s[2]] + g[128:193] + [s[3]] + g[193:493] + g[100:110] + g[110:120],
              [s[4], small[0], s[5], small[1], s[6], small[2], s[7], small[3], s[8], small[4], s[9]], [z, w, s[10]], list(big),
              [s[11]] + g[493:500], []]
    offsets, at = [], 5
    for cs in chunks:
        offsets.append(at)
        at += sum(sizes[c] for c in cs) + 7
    small_start = np.concatenate([[0], np.cumsum([sizes[c] for c in small])]).tolist()
    suffixes = (0, 1, 5, 7)
    assert {(base_offsets[1] + small_start[k]) % 4 for k in suffixes} == {0, 1, 2, 3}
    for r in range(16):
        for k in suffixes:
            names.append(f"t/r{r:02d}k{k}")
            chunks.append(small[k:])
            offsets.append((at + 15) // 16 * 16 + r)
            at = offsets[-1] + sum(sizes[c] for c in small[k:])
    out_bytes = at + 9
    vi = version_of(hash_id, names, chunks, hashes, sizes)
    files = [np.concatenate([pool[c] for c in cs]) if cs else np.zeros(0, np.uint8) for cs in chunks]
    # ---- the store: two blocks of what the base cannot feed, one block of chunks the base holds too ----
    block_chunks = [s[:6] + [z], s[6:] + [w], [g[0], g[1], small[4]]]
    blocks = [(0xB10C0 + b, 0, cs) for b, cs in enumerate(block_chunks)]
    si = build_store_index(hash_id, blocks, hashes, sizes)
    images = [raw_image(bh, hash_id, [hashes[c] for c in cs], [sizes[c] for c in cs], np.concatenate([pool[c] for c in cs])) for bh, _, cs in blocks]
    return dict(vi=vi, si=si, images=images, offsets=np.array(offsets, np.uint64), out_bytes=out_bytes, files=files, base_vi=base_vi,
                base_offsets=np.array(base_offsets, np.uint64), base_bytes=base_bytes, base_host=base_host, needed=[0xB10C0, 0xB10C1])


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("hash_id", [BLK3, BLK2, MEOW])
def test_runs_and_alignments_on_versions_built_by_hand(gpu, hash_id, verify):
    c = sweep_case(gpu, hash_id)
    occ = occurrences(c["vi"], c["offsets"])
    places = first_places(c["base_vi"], c["base_offsets"])
    fed = fed_by(places, occ)
    pairs = {(at % 16, places[h][0] % 4) for h, at, _ in fed}
    assert pairs == {(d, q) for d in range(16) for q in range(4)}, "every destination residue mod 16 against every source residue mod 4"
    assert max(sum(1 for o in fed if o[0] == h) for h in {o[0] for o in fed}) >= 16, "one base chunk feeds many occurrences"
    base_dev = torch.from_numpy(c["base_host"]).cuda()
    assert base_dev.numel() == c["base_bytes"]
    code, res, out, needed = update(gpu, (c["vi"], c["offsets"]), (c["si"], c["images"]),
                                    (c["base_vi"], c["base_offsets"], c["base_bytes"], base_dev), c["out_bytes"], verify=verify)
    assert code == 0
    assert needed == c["needed"] == blocks_with_a_chunk_outside(c["si"], places, occ)
    want = expected_output(c["files"], c["offsets"], c["out_bytes"])
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])
    total = sum(len(f) for f in c["files"])
    assert (res.occurrences, res.base_occurrences, res.base_bytes) == (len(occ), len(fed), sum(n for _, _, n in fed))
    assert 0 < res.base_occurrences < res.occurrences
    assert (res.occurrences_written, res.bytes_written) == (len(occ), total)
    assert (res.blocks_needed, res.blocks_bad, res.chunks_mismatched, res.base_chunks_mismatched) == (2, 0, 0, 0)


# ---- what the stream session wrote for version A, and for version B with and without a store that holds A: once per configuration ----


def versions(gpu, oracle, ref, cfg):
    """dict(a, b_missing, b_full: dict(vi, si, images), files_a, files_b, base: A restored by the plain session (host), and its layout)"""
    if cfg in _runs:
        return _runs[cfg]
    target, codec, max_block, max_chunks = cfg
    tag = tag_of(ref, codec)
    tree_a, tree_b = tree_of(oracle, ref, target), next_version(oracle, ref, target)

    def run(tree, store):
        r = store_tests.run_stream(gpu, tree, target, codec, max_block, max_chunks, tag, slices_of("three", tree["part"].job_count), store)
        return dict(vi=r["vi"], si=r["si"], images=[i for _, imgs in r["calls"] for i in imgs])

    store = store_tests.keep(Store(gpu, 0))
    a = run(tree_a, store)
    store.add_index(a["si"])
    b_missing, b_full = run(tree_b, store), run(tree_b, None)
    assert b_full["vi"] == b_missing["vi"]
    files_a, files_b = files_of(tree_a), files_of(tree_b)
    offsets_a, total_a = Restore.layout(a["vi"], 64)
    rs = keep(Restore(gpu, a["vi"], a["si"], offsets_a, total_a, verify=True))
    out = torch.full((total_a,), FILL, dtype=torch.uint8, device="cuda")
    deliver(rs, parse_store_index(a["si"])["block_hashes"], a["images"], out)
    code, _ = rs.finish()
    base = out.cpu().numpy()
    assert code == 0 and (base == expected_output(files_a, offsets_a, total_a)).all()
    offsets_b, total_b = Restore.layout(b_full["vi"], 64)
    _runs[cfg] = dict(a=a, b_missing=b_missing, b_full=b_full, files_a=files_a, files_b=files_b, base=base, offsets_a=offsets_a,
                      total_a=total_a, offsets_b=offsets_b, total_b=total_b)
    for held in (_open, store_tests._open, _sessions):
        while held:
            held.pop().close()
    return _runs[cfg]


def base_of(v, host=None):
    return (v["a"]["vi"], v["offsets_a"], v["total_a"], torch.from_numpy(v["base"] if host is None else host).cuda())


# ---- 2. version A -> version B ----


@pytest.mark.parametrize("verify", [False, True])
@pytest.mark.parametrize("cfg", STORE_CONFIGS)
def test_the_next_version_from_the_base_and_the_blocks_it_added(gpu, oracle, ref, cfg, verify):
    v = versions(gpu, oracle, ref, cfg)
    b = v["b_missing"]
    all_blocks = [int(h) for h in parse_store_index(b["si"])["block_hashes"]]
    assert all_blocks
    refused(errno.ENOENT, lambda: Restore(gpu, b["vi"], b["si"], v["offsets_b"], v["total_b"]))  # the plain session cannot
    code, res, out, needed = update(gpu, (b["vi"], v["offsets_b"]), (b["si"], b["images"]), base_of(v), v["total_b"], verify=verify)
    assert code == 0 and needed == all_blocks
    want = expected_output(v["files_b"], v["offsets_b"], v["total_b"])
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])
    assert res.base_occurrences * 2 > res.occurrences, "most of version B comes from the base"
    assert res.occurrences_written == res.occurrences and res.bytes_written == sum(len(f) for f in v["files_b"])
    assert res.blocks_needed == res.blocks_delivered == len(all_blocks) and res.blocks_bad == res.base_chunks_mismatched == 0


# ---- 3. the base wins ----


@pytest.mark.parametrize("cfg", STORE_CONFIGS)
def test_the_base_wins_over_the_store(gpu, oracle, ref, cfg):
    v = versions(gpu, oracle, ref, cfg)
    b = v["b_full"]
    occ = occurrences(b["vi"], v["offsets_b"])
    want_needed = blocks_with_a_chunk_outside(b["si"], first_places(v["a"]["vi"], v["offsets_a"]), occ)
    assert 0 < len(want_needed) < len(parse_store_index(b["si"])["block_hashes"])
    code, res, out, needed = update(gpu, (b["vi"], v["offsets_b"]), (b["si"], b["images"]), base_of(v), v["total_b"])
    assert needed == want_needed
    assert code == 0 and res.blocks_needed == res.blocks_delivered == len(want_needed)
    want = expected_output(v["files_b"], v["offsets_b"], v["total_b"])
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])


# ---- 4. a partial base, a partial target ----


def test_a_base_of_which_every_second_asset_is_resident(gpu, oracle, ref):
    v = versions(gpu, oracle, ref, STORE_CONFIGS[0])
    b = v["b_full"]
    offsets_a = np.array([o if a % 2 == 0 else Restore.SKIP for a, o in enumerate(v["offsets_a"].tolist())], np.uint64)
    host = v["base"].copy()
    for a, (o, f) in enumerate(zip(v["offsets_a"].tolist(), v["files_a"])):
        if a % 2:
            host[o : o + len(f)] = 0x77  # what is not resident is not read
    occ = occurrences(b["vi"], v["offsets_b"])
    want_needed = blocks_with_a_chunk_outside(b["si"], first_places(v["a"]["vi"], offsets_a), occ)
    whole = blocks_with_a_chunk_outside(b["si"], first_places(v["a"]["vi"], v["offsets_a"]), occ)
    assert len(want_needed) > len(whole), "a smaller base needs more blocks"
    base = (v["a"]["vi"], offsets_a, v["total_a"], torch.from_numpy(host).cuda())
    code, res, out, needed = update(gpu, (b["vi"], v["offsets_b"]), (b["si"], b["images"]), base, v["total_b"])
    assert needed == want_needed and code == 0
    want = expected_output(v["files_b"], v["offsets_b"], v["total_b"])
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])


def test_only_what_version_diff_says_changed(gpu, oracle, ref):
    v = versions(gpu, oracle, ref, STORE_CONFIGS[1])
    b = v["b_missing"]
    removed, added, _, content, _, _ = version_diff(v["a"]["vi"], b["vi"])
    names_a, names_b = asset_fields(v["a"]["vi"])["names"], asset_fields(b["vi"])["names"]
    assert [names_a[i] for i in removed] == ["dir2/sub1/file05.bin"]
    assert "dir1/added.bin" in [names_b[i] for i in added]
    assert sorted(names_b[i] for i in content) == ["dir1/sub0/file10.bin", "dir1/sub1/file01.bin"]
    selected = set(added.tolist()) | set(content.tolist())
    offsets, at = [], 3
    for a, f in enumerate(v["files_b"]):
        offsets.append(at if a in selected else Restore.SKIP)
        at += len(f) + 1 if a in selected else 0
    offsets, pad = np.array(offsets, np.uint64), 4096
    code, res, out, _ = update(gpu, (b["vi"], offsets), (b["si"], b["images"]), base_of(v), at, pad=pad)
    assert code == 0 and res.assets_selected == len(selected)
    want = expected_output(v["files_b"], offsets, at + pad)
    assert (out == want).all(), int(np.flatnonzero(out != want)[0])
    assert res.bytes_written == sum(len(v["files_b"][a]) for a in selected) and 0 < res.base_bytes < res.bytes_written


# ---- 5. a damaged base ----


def test_a_damaged_base_chunk(gpu, oracle, ref):
    v = versions(gpu, oracle, ref, STORE_CONFIGS[0])
    b = v["b_missing"]
    occ = occurrences(b["vi"], v["offsets_b"])
    places = first_places(v["a"]["vi"], v["offsets_a"])
    fed = fed_by(places, occ)
    victim = next(h for h, _, n in fed[len(fed) // 2 :] if n > 8)  # a chunk in the middle of what the base feeds
    hit = [(at, n) for h, at, n in fed if h == victim]
    host = v["base"].copy()
    host[places[victim][0] + 3] ^= 0x40
    want = expected_output(v["files_b"], v["offsets_b"], v["total_b"])
    # ---- verify: the chunk's occurrences keep what the output held, everything else is right ----
    code, res, out, _ = update(gpu, (b["vi"], v["offsets_b"]), (b["si"], b["images"]), base_of(v, host), v["total_b"], verify=True)
    assert code == errno.EBADF and res.base_chunks_mismatched == 1 and res.blocks_bad == 0
    kept = want.copy()
    for at, n in hit:
        kept[at : at + n] = FILL
    assert (out == kept).all(), int(np.flatnonzero(out != kept)[0])
    assert res.occurrences_written == res.occurrences - len(hit)
    assert res.bytes_written == sum(len(f) for f in v["files_b"]) - sum(n for _, n in hit)
    # ---- without verify the base is trusted: the flipped byte arrives ----
    code, res, out, _ = update(gpu, (b["vi"], v["offsets_b"]), (b["si"], b["images"]), base_of(v, host), v["total_b"], verify=False)
    assert code == 0 and res.base_chunks_mismatched == 0 and res.occurrences_written == res.occurrences
    assert np.flatnonzero(out != want).tolist() == sorted(at + 3 for at, _ in hit)
    assert all(int(out[at + 3]) == int(want[at + 3]) ^ 0x40 for at, _ in hit)


# ---- 6. order and refusals ----


def test_carry_in_any_order_with_the_blocks_calls(gpu, oracle, ref):
    v = versions(gpu, oracle, ref, STORE_CONFIGS[1])
    b = v["b_missing"]
    want = expected_output(v["files_b"], v["offsets_b"], v["total_b"])
    for carry_at in (0, 1, 2):
        code, res, out, needed = update(gpu, (b["vi"], v["offsets_b"]), (b["si"], b["images"]), base_of(v), v["total_b"], carry_at=carry_at)
        assert code == 0 and len(needed) >= 2, carry_at
        assert (out == want).all(), (carry_at, int(np.flatnonzero(out != want)[0]))


def test_refusals_leave_the_session_and_the_context_usable(gpu, oracle, ref):
    v = versions(gpu, oracle, ref, STORE_CONFIGS[0])
    a, b = v["a"], v["b_missing"]
    want = expected_output(v["files_b"], v["offsets_b"], v["total_b"])
    base = base_of(v)
    target = (b["vi"], b["si"], v["offsets_b"], v["total_b"])
    # ---- from create ----
    other_id = np.frombuffer(a["vi"], np.uint8).copy()
    other_id[4:8] = np.array([BLK2], np.uint32).view(np.uint8)
    refused(errno.EINVAL, lambda: Restore(gpu, *target, base=(other_id.tobytes(), v["offsets_a"], v["total_a"])))
    refused(errno.EINVAL, lambda: Restore(gpu, *target, base=(a["vi"], v["offsets_a"], v["total_a"] - 1)))  # the last window leaves the base
    refused(errno.EBADF, lambda: Restore(gpu, *target, base=(a["vi"][:-1], v["offsets_a"], v["total_a"])))
    raw_a, raw_b, raw_s = (np.frombuffer(x, np.uint8) for x in (a["vi"], b["vi"], b["si"]))
    cfg = RestoreConfig(C.sizeof(RestoreConfig), 1)
    short = RestoreBase(8, raw_a.ctypes.data, len(raw_a), v["offsets_a"].ctypes.data, v["total_a"])
    h = C.c_void_p()
    assert gpu.lib.dll.lthip_restore_create_from_base(gpu.h, C.byref(cfg), C.byref(short), raw_b.ctypes.data, len(raw_b), raw_s.ctypes.data,
                                                      len(raw_s), v["offsets_b"].ctypes.data, v["total_b"], C.byref(h)) == errno.EINVAL
    assert not h.value
    # ---- from carry and finish: nothing is queued, nothing changes ----
    rs = keep(Restore(gpu, *target, verify=True, base=base[:3]))
    hashes = parse_store_index(b["si"])["block_hashes"]
    both = torch.full((v["total_a"] + v["total_b"],), FILL, dtype=torch.uint8, device="cuda")
    both[: v["total_a"]] = base[3]
    out = torch.full((v["total_b"],), FILL, dtype=torch.uint8, device="cuda")
    deliver(rs, hashes, b["images"], out)
    code, res = rs.finish()
    assert code == errno.ENOENT and res.blocks_delivered == res.blocks_needed, "every block is there, the base is not"
    refused(errno.EINVAL, lambda: rs.carry(None, out))
    refused(errno.EINVAL, lambda: rs.carry(base[3], None))
    refused(errno.EINVAL, lambda: rs.carry(both[: v["total_a"]], both[v["total_a"] - 16 :]))  # the output starts inside the base
    refused(errno.EINVAL, lambda: rs.carry(both[16 : 16 + v["total_a"]], both[:16]))            # the base starts inside the output
    assert rs.finish()[0] == errno.ENOENT
    rs.carry(base[3], out)
    refused(errno.EEXIST, lambda: rs.carry(base[3], out))
    code, res = rs.finish()
    assert code == 0 and res.occurrences_written == res.occurrences
    got = out.cpu().numpy()
    assert (got == want).all(), int(np.flatnonzero(got != want)[0])
    # ---- a session without a base has nothing to carry, and restores as it always did ----
    plain = keep(Restore(gpu, a["vi"], a["si"], v["offsets_a"], v["total_a"], verify=True))
    out_a = torch.full((v["total_a"],), FILL, dtype=torch.uint8, device="cuda")
    refused(errno.EINVAL, lambda: plain.carry(base[3], out_a))
    deliver(plain, parse_store_index(a["si"])["block_hashes"], a["images"], out_a)
    code, res = plain.finish()
    assert code == 0 and (res.base_occurrences, res.base_bytes, res.base_chunks_mismatched) == (0, 0, 0)
    assert (out_a.cpu().numpy() == v["base"]).all()
