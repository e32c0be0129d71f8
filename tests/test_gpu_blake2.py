"""-m gpu: the 'blk2' hash type (BLAKE2s-64, lib/blake2/longtail_blake2.c) against hashlib.blake2s(digest_size=8) -- the reference's
blake2s(out, 8, data, len, 0, 0) read as a little-endian u64 -- and, through the reference core (oracle/_ref), the VersionIndex /
StoreIndex a 'blk2' store holds:

  * lthip_blake2s_ranges[_dev], _one, _runs_u64, the streaming pair: digests == hashlib, lengths around every block boundary, any
    start offset, overlapping ranges, 1 .. 200 000 ranges, the device count behind lthip_chunk_hash(d_chunk_hashes = NULL)
  * Longtail_CreateHipBlake2HashAPI: identifier 'blk2', the five entry points, found by Longtail_CreateDefaultHashRegistry
  * Longtail_CreateVersionIndex with HIP chunker + HIP BLAKE2 and with the reference chunker + HIP BLAKE2 == with a hashlib HashAPI
  * the bulk session with hash_identifier 'blk2': VersionIndex and StoreIndex byte for byte, stored blocks open with the reference
  * BLAKE3 results of the same calls are unchanged (the dispatch by identifier keeps the 'blk3' path)"""
import ctypes as C
import errno
import hashlib

import numpy as np
import pytest
import torch

from longtail_amd.dist import JobPartition
from longtail_amd.lib import HASH_BLAKE2, HASH_BLAKE3, Context, Ingest, chunker_params
from tests.gpu_util import dev_u32, dev_u64, to_device, u32, u64
from tests.test_gpu_ingest import make_files, parse_store_index, ref_missing_content, version_unique_lists
from tests.test_gpu_plugins import ChunkerAPIStruct, CompressionAPIStruct, HashAPIStruct, PyHashAPI

pytestmark = pytest.mark.gpu


def b2(data) -> int:
    return int.from_bytes(hashlib.blake2s(bytes(data), digest_size=8).digest(), "little")


@pytest.fixture(scope="module")
def gpu():
    ctx = Context(0)
    yield ctx
    ctx.close()


def check_ranges(gpu, host, offs, lens, max_len=0, **kw):
    dev = torch.from_numpy(host).cuda()
    got = u64(gpu.blake2s_ranges(dev, dev_u64(offs), dev_u32(lens), max_len, **kw))
    exp = np.array([b2(host[o : o + n]) for o, n in zip(offs, lens)], np.uint64)
    bad = np.nonzero(got[: len(exp)] != exp)[0]
    assert len(bad) == 0, [(int(offs[i]), int(lens[i])) for i in bad[:8]]


def test_ranges_lengths_and_offsets(gpu):
    rng = np.random.default_rng(2)
    host = rng.integers(0, 256, size=(1 << 20) + 64, dtype=np.uint8)
    special = [0, 1, 55, 56, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]
    offs, lens = [], []
    for n in special:
        for r in range(16):  # every start residue mod 16
            offs.append(1000 + 16 * int(rng.integers(0, 100)) + r)
            lens.append(n)
    check_ranges(gpu, host, offs, lens)             # few ranges: the quad kernel
    check_ranges(gpu, host, offs * 3, lens * 3, 4097)  # > 256 ranges (sorted lane kernel), max_len exact, duplicated ranges
    for count in (1, 2, 257):
        o = rng.integers(0, 700000, size=count)
        n = rng.integers(0, 300000, size=count)
        check_ranges(gpu, host, o, n)  # overlapping random ranges up to 300 000 bytes


def test_ranges_many(gpu):
    rng = np.random.default_rng(3)
    host = rng.integers(0, 256, size=(4 << 20) + 64, dtype=np.uint8)
    count = 200000
    o = rng.integers(0, 4 << 20, size=count)
    n = np.minimum(rng.integers(0, 3000, size=count), (4 << 20) - o)
    n[::997] = 0
    check_ranges(gpu, host, o, n)
    o2 = rng.integers(0, 1 << 20, size=1500)
    n2 = rng.integers(0, 300000, size=1500)
    check_ranges(gpu, host, o2, n2, 300000)


@pytest.mark.parametrize("source", ["golden", "synth64"])
def test_ranges_device_count_behind_the_chunker(gpu, golden, oracle, source):
    if source == "golden":
        data = golden["chunker_input"]
        target = 4096
    else:
        data = oracle.synth(64 << 20, 11, 1)
        target = 65536
    mn, av, mx = chunker_params(target)
    dev, offs = to_device([data])
    plan = gpu.make_plan(offs, [len(data)], mn, av, mx)
    total, d_off, d_len, d_hash, d_first = gpu.chunk_hash(plan, dev, want_hashes=False, sync=False)
    cap = plan.capacity
    out = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
    gpu.blake2s_ranges(dev, d_off, d_len, mx, out=out, count_bound=cap, d_count=d_first[1:])
    n = int(u32(d_first)[1])
    got = u64(out)
    ho, hl = u64(d_off)[:n], u32(d_len)[:n]
    exp = np.array([b2(data[o : o + k]) for o, k in zip(ho, hl)], np.uint64)
    assert (got[:n] == exp).all()
    assert (got[n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "slots beyond the device count were written"
    # the BLAKE3 digests of the same chunks are untouched by the new path
    _, _, _, d_h3, _ = gpu.chunk_hash(plan, dev)
    assert (u64(d_h3)[:n] == np.array([oracle.blake3(data[o : o + k]) for o, k in zip(ho, hl)], np.uint64)).all()
    plan.close()


def test_one_every_length(gpu):
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, size=65536 + 16, dtype=np.uint8)
    pin = torch.from_numpy(src.copy()).pin_memory()
    out = torch.zeros(1, dtype=torch.int64).pin_memory()
    dev = torch.from_numpy(src.copy()).cuda()
    dout = torch.zeros(1, dtype=torch.int64, device="cuda")
    for n in list(range(0, 1025)) + [4096, 65535, 65536]:
        gpu.blake2s_one(pin, n, out)
        gpu.sync()
        assert int(out.numpy().view(np.uint64)[0]) == b2(src[:n]), n
    for n in (0, 1, 100, 65536):
        gpu.blake2s_one(dev, n, dout)
        assert int(u64(dout)[0]) == b2(src[:n]), n
    gpu.blake2s_one(pin[1:], 777, out)  # an unaligned start
    gpu.sync()
    assert int(out.numpy().view(np.uint64)[0]) == b2(src[1:778])
    assert gpu.lib.dll.lthip_blake2s_one(gpu.h, pin.data_ptr(), 65537, out.data_ptr()) == errno.EINVAL


def test_runs_u64(gpu):
    rng = np.random.default_rng(5)
    vals = rng.integers(0, 2**63, size=(1 << 20) + 10, dtype=np.int64).view(np.uint64)
    d_vals = dev_u64(vals)
    first = np.array([0, 0, 3, 3 + (1 << 20), (1 << 20) + 10], np.uint32)  # an empty run, 3 values, 2^20 values, 7 values
    got = u64(gpu.blake2s_runs_u64(d_vals, dev_u32(first), len(first) - 1))
    exp = [b2(vals[first[i] : first[i + 1]].tobytes()) for i in range(len(first) - 1)]
    assert list(got) == exp
    assert gpu.lib.dll.lthip_blake2s_runs_u64(gpu.h, d_vals.data_ptr(), dev_u32(first).data_ptr(), 0, d_vals.data_ptr()) == 0


def test_stream(gpu):
    rng = np.random.default_rng(6)
    B = 1 << 20
    host = rng.integers(0, 256, size=3 * B + 64, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    for n in (0, 1, 63, 64, 65, 300000, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1, 3 * B):
        assert gpu.b2s_stream(dev, n) == b2(host[:n]), n
    big = torch.randint(0, 256, (256 << 20,), dtype=torch.uint8, device="cuda")
    h = hashlib.blake2s(digest_size=8)
    h.update(big.cpu().numpy().tobytes())
    assert gpu.b2s_stream(big, 256 << 20) == int.from_bytes(h.digest(), "little")


# ---- the HashAPI object ----
@pytest.fixture(scope="module")
def hip_b2(hiplib):
    p = hiplib.dll.Longtail_CreateHipBlake2HashAPI()
    assert p
    yield p
    HashAPIStruct.from_address(p).Dispose(p)


def test_hash_api_entry_points(hip_b2):
    h = HashAPIStruct.from_address(hip_b2)
    assert h.GetIdentifier(hip_b2) == HASH_BLAKE2 == 0x626C6B32
    out = C.c_uint64(0)
    assert h.HashBuffer(hip_b2, 0, b"\0", C.byref(out)) == 0 and out.value == b2(b"")
    data = np.random.default_rng(7).integers(0, 256, size=(2 << 20) + 3, dtype=np.uint8)
    for n in (1, 63, 64, 65, 1024, 65536, 70000, 300000, 2 << 20):
        assert h.HashBuffer(hip_b2, n, data.ctypes.data, C.byref(out)) == 0
        assert out.value == b2(data[:n]), n
    for cuts in ([], [0], [1], [63, 64, 65], [1000, 150000], [(1 << 20) - 1, (1 << 20) + 1], [1 << 20], [5, (2 << 20) + 3]):
        ctx = C.c_void_p()
        assert h.BeginContext(hip_b2, C.byref(ctx)) == 0
        pts = [0] + cuts + [len(data)]
        for a, b in zip(pts, pts[1:]):
            h.Hash(hip_b2, ctx, b - a, data.ctypes.data + a)
        assert h.EndContext(hip_b2, ctx) == b2(data), cuts
    ctx = C.c_void_p()
    assert h.BeginContext(hip_b2, C.byref(ctx)) == 0
    assert h.EndContext(hip_b2, ctx) == b2(b"")  # the empty stream


# a hashlib-backed Longtail_HashAPI: the reference core with it builds the reference's BLAKE2 VersionIndex
@pytest.fixture(scope="module")
def py_b2():
    return PyHashAPI(HASH_BLAKE2, b2)


@pytest.mark.parametrize("workers", [0, 4])
def test_reference_version_index_with_hip_blake2(ref, oracle, hiplib, hip_b2, py_b2, workers):
    files = make_files(oracle, 1024)
    expect, _ = ref.version_index(files, 1024, workers, ref.lz4_type, hash_api=py_b2.ptr)
    assert np.frombuffer(expect[:8], np.uint32)[1] == HASH_BLAKE2
    got_ref_chunker, _ = ref.version_index(files, 1024, workers, ref.lz4_type, hash_api=hip_b2)
    assert got_ref_chunker == expect
    chunker = hiplib.dll.Longtail_CreateHipChunkerAPI()
    try:
        got_hip, _ = ref.version_index(files, 1024, workers, ref.lz4_type, chunker_api=chunker, hash_api=hip_b2)
    finally:
        ChunkerAPIStruct.from_address(chunker).Dispose(chunker)
    assert got_hip == expect


def test_hash_registry_returns_the_blake2_object(ref, hiplib):
    d = ref.dll
    d.Longtail_CreateDefaultHashRegistry.restype = C.c_void_p
    d.Longtail_CreateDefaultHashRegistry.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    d.Longtail_GetHashRegistry_GetHashAPI.restype = C.c_int
    d.Longtail_GetHashRegistry_GetHashAPI.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    h3, h2 = hiplib.dll.Longtail_CreateHipBlake3HashAPI(), hiplib.dll.Longtail_CreateHipBlake2HashAPI()
    types = (C.c_uint32 * 2)(HASH_BLAKE3, HASH_BLAKE2)
    apis = (C.c_void_p * 2)(h3, h2)
    reg = d.Longtail_CreateDefaultHashRegistry(2, types, apis)
    assert reg
    out = C.c_void_p()
    assert d.Longtail_GetHashRegistry_GetHashAPI(reg, HASH_BLAKE2, C.byref(out)) == 0 and out.value == h2
    assert HashAPIStruct.from_address(out.value).GetIdentifier(out.value) == HASH_BLAKE2
    assert d.Longtail_GetHashRegistry_GetHashAPI(reg, HASH_BLAKE3, C.byref(out)) == 0 and out.value == h3
    HashAPIStruct.from_address(reg).Dispose(reg)  # (a Longtail_API first, like every longtail object)


def test_ingest_roundtrip_through_hip_objects(ref, oracle, hiplib, hip_b2):
    files = make_files(oracle, 1024)[:8]
    chunker = hiplib.dll.Longtail_CreateHipChunkerAPI()
    lz4 = hiplib.dll.Longtail_CreateHipLZ4CompressionAPI()
    try:
        err = ref.ingest_roundtrip(files, 1024, 262144, 64, ref.lz4_type, 0, chunker_api=chunker, hash_api=hip_b2, codec_api=lz4)
    finally:
        ChunkerAPIStruct.from_address(chunker).Dispose(chunker)
        CompressionAPIStruct.from_address(lz4).Dispose(lz4)
    assert err["err"] == 0 and err["chunks"] > 0 and err["blocks"] > 0, err


# ---- the bulk session with hash_identifier 'blk2' ----
def b2_session(gpu, ref, files, target, max_block, max_chunks, tag, hash_identifier):
    paths, sizes, offs, perms, path_data = ref.tree_file_infos(files)
    by_name = {n: d for n, d in files}
    part = JobPartition(sizes, target, 1, "range")
    blobs = []
    for j in range(part.job_count):
        data = by_name.get(paths[int(part.job_asset[j])], np.zeros(0, np.uint8))
        o, s = int(part.job_offset[j]), int(part.job_size[j])
        blobs.append(data[o : o + s])
    dev, part_offs = to_device(blobs)
    mn, av, mx = chunker_params(target)
    plan = gpu.make_plan(part_offs, [len(b) for b in blobs], mn, av, mx)
    if hash_identifier == HASH_BLAKE2:
        total, d_off, d_len, _, d_first = gpu.chunk_hash(plan, dev, want_hashes=False)
        d_hash = torch.empty(max(1, plan.capacity), dtype=torch.int64, device="cuda")
        gpu.blake2s_ranges(dev, d_off, d_len, mx, out=d_hash, count_bound=plan.capacity, d_count=d_first[plan.nparts:])
    else:
        total, d_off, d_len, d_hash, d_first = gpu.chunk_hash(plan, dev)
    plan.close()
    first = u32(d_first).astype(np.int64)
    job_first = first.astype(np.uint64)
    ing = Ingest(gpu, target, max_block, max_chunks, "lz4", compression_type=tag, hash_identifier=hash_identifier)
    tree, keep = Ingest.tree(sizes.copy(), offs.copy(), perms.copy(), path_data, part.job_asset.copy(), job_first.copy())
    vi = torch.zeros(gpu.lib.dll.lthip_version_index_size(len(sizes), total, total, len(path_data)) + 64, dtype=torch.uint8).pin_memory()
    ing.index(tree, d_hash[:total], d_len[:total], total, d_off, d_first, total, vi)
    arena = torch.zeros(96 << 20, dtype=torch.uint8, device="cuda")
    ing.write(dev, arena)
    si = torch.zeros(16 + 32 * max(total, 1) + 64, dtype=torch.uint8).pin_memory()
    res = ing.finish(si)
    return dict(vi=bytes(vi.numpy()[: res.version_index_size]), si=bytes(si.numpy()[: res.store_index_size]), res=res, ing=ing, arena=arena,
                comp=ing.compressed_sizes(res.blocks), all_hash=d_hash[:total], dev=dev, d_off=d_off, d_len=d_len, d_hash=d_hash, total=total)


def expected_b2_store_index(ref, expect_vi, max_block, max_chunks):
    uh, us, ut = version_unique_lists(expect_vi)
    si = bytearray(ref_missing_content(ref, np.zeros(0, np.uint64), uh, us, ut, max_block, max_chunks))
    np.frombuffer(si, np.uint32, 1, 4)[:] = HASH_BLAKE2
    p = parse_store_index(bytes(si))
    nb = len(p["block_hashes"])
    starts = np.concatenate([[0], np.cumsum(p["block_counts"])]).astype(np.int64)
    for b in range(nb):
        chunk_bytes = p["chunk_hashes"][starts[b] : starts[b + 1]].tobytes()  # src/longtail.c:3757: hash of the block's chunk hashes
        np.frombuffer(si, np.uint64, 1, 16 + 8 * b)[:] = b2(chunk_bytes)
    return bytes(si)


def check_b2_images(gpu, ref, sess, tag):
    """Every stored-block image: its BlockIndex carries 'blk2' and the BLAKE2 hash of the block's chunk hashes (src/longtail.c:3757);
    with those two fields set to what a 'blk3' block would carry, the reference's reader opens it and its codec decodes the payload to
    the chunks' bytes (refh_open_stored_block compares against a BLAKE3 BlockIndex)."""
    si = parse_store_index(sess["si"])
    _, offs, sizes = sess["ing"].images()
    arena = sess["arena"].cpu().numpy()
    data = sess["dev"].cpu().numpy()
    l_off, l_len, l_hash = (u64(sess["d_off"])[: sess["total"]], u32(sess["d_len"])[: sess["total"]], u64(sess["d_hash"])[: sess["total"]])
    where = {}
    for k in range(sess["total"]):
        where.setdefault(int(l_hash[k]), (int(l_off[k]), int(l_len[k])))
    assert len(offs) == sess["res"].blocks > 0
    for b in range(len(offs)):
        c0, n = int(si["block_offsets"][b]), int(si["block_counts"][b])
        h = np.ascontiguousarray(si["chunk_hashes"][c0 : c0 + n])
        s = np.ascontiguousarray(si["chunk_sizes"][c0 : c0 + n])
        image = arena[int(offs[b]) : int(offs[b]) + int(sizes[b])].copy()
        head = np.frombuffer(image[:20].tobytes(), np.uint32)
        assert int(head[0]) | (int(head[1]) << 32) == b2(h.tobytes()) == int(si["block_hashes"][b]), b
        assert head[2] == HASH_BLAKE2 and head[3] == n and head[4] == tag, b
        image[:8] = np.frombuffer(np.uint64(ref.blake3(np.frombuffer(h.tobytes(), np.uint8))).tobytes(), np.uint8)
        image[8:12] = np.frombuffer(np.uint32(HASH_BLAKE3).tobytes(), np.uint8)
        raw = int(s.astype(np.int64).sum())
        out = np.zeros(raw + 8, np.uint8)
        got = C.c_uint64(0)
        err = ref.dll.refh_open_stored_block(image.ctypes.data, len(image), n, h.ctypes.data, s.ctypes.data, tag, out.ctypes.data, raw,
                                             C.byref(got))
        assert err == 0, (b, err)
        expect = np.concatenate([data[where[int(x)][0] : where[int(x)][0] + where[int(x)][1]] for x in h])
        assert got.value == raw and (out[:raw] == expect).all(), b


@pytest.mark.parametrize("target,max_block,max_chunks", [(1024, 262144, 16), (65536, 8 << 20, 1024)])
def test_ingest_session_blk2_matches_reference(gpu, oracle, ref, py_b2, target, max_block, max_chunks):
    files = make_files(oracle, target)
    tag = ref.lz4_type
    sess = b2_session(gpu, ref, files, target, max_block, max_chunks, tag, HASH_BLAKE2)
    expect_vi, _ = ref.version_index(files, target, 0, tag, hash_api=py_b2.ptr)
    assert sess["vi"] == expect_vi, "BLAKE2 VersionIndex differs from Longtail_CreateVersionIndex with a BLAKE2 HashAPI"
    assert sess["si"] == expected_b2_store_index(ref, expect_vi, max_block, max_chunks)
    check_b2_images(gpu, ref, sess, tag)
    sess["ing"].close()
    # ... and 'blk3' still gives the reference's BLAKE3 index
    s3 = b2_session(gpu, ref, files, target, max_block, max_chunks, tag, HASH_BLAKE3)
    assert s3["vi"] == ref.version_index(files, target, 0, tag)[0]
    s3["ing"].close()


def test_blake2s_allocation_failures_report_enomem(hiplib):
    from longtail_amd.lib import load_ablations

    abl = load_ablations()
    ctx = Context(0, lib=abl)
    d = abl.dll
    n = 5000
    data = torch.randint(0, 256, (1 << 20,), dtype=torch.uint8, device="cuda")
    offs = dev_u64(np.arange(n) * 100)
    lens = dev_u32(np.full(n, 100))
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    try:
        assert d.lthip_debug_fail_alloc(0, 1) == 0
        err = d.lthip_blake2s_ranges(ctx.h, data.data_ptr(), n, offs.data_ptr(), lens.data_ptr(), 0, out.data_ptr())
        assert err == errno.ENOMEM, err
    finally:
        d.lthip_debug_fail_alloc(-1, 0)
    assert d.lthip_blake2s_ranges(ctx.h, data.data_ptr(), n, offs.data_ptr(), lens.data_ptr(), 0, out.data_ptr()) == 0
    ctx.sync()
    host = data.cpu().numpy()
    assert int(u64(out)[7]) == b2(host[700:800])
    ctx.close()


def test_ranges_long_ones_among_many(gpu):
    """> 256 ranges with some of them >= 1 MiB: the longest length classes run on quads, the rest one lane per range."""
    rng = np.random.default_rng(8)
    host = rng.integers(0, 256, size=(12 << 20) + 64, dtype=np.uint8)
    o = list(rng.integers(0, 1 << 20, size=400))
    n = list(rng.integers(0, 5000, size=400))
    for k, (off, ln) in enumerate([(3, 8 << 20), (17, (1 << 20) - 1), (64, 1 << 20), (5, (1 << 20) + 63), (1000, 3 << 20)]):
        o.insert(37 * k, off)  # among the short ones, not first
        n.insert(37 * k, ln)
    check_ranges(gpu, host, o, n)
    first = np.array([0, 1 << 20, (1 << 20) + 3] + [(1 << 20) + 3 + 10 * k for k in range(1, 300)], np.uint32)  # runs: 2^20 values, then 300 short
    vals = host[: 8 * int(first[-1])].view(np.uint64)
    got = u64(gpu.blake2s_runs_u64(dev_u64(vals), dev_u32(first), len(first) - 1))
    assert list(got) == [b2(vals[first[i] : first[i + 1]].tobytes()) for i in range(len(first) - 1)]


def test_one_any_alignment(gpu):
    src = np.random.default_rng(9).integers(0, 256, size=65536 + 64, dtype=np.uint8)
    pin = torch.from_numpy(src.copy()).pin_memory()
    out = torch.zeros(1, dtype=torch.int64).pin_memory()
    for start in range(16):
        for n in (0, 1, 15, 16, 17, 63, 64, 65, 1000, 65536 - 16, 65536):
            gpu.blake2s_one(pin[start:], n, out)
            gpu.sync()
            assert int(out.numpy().view(np.uint64)[0]) == b2(src[start : start + n]), (start, n)


def test_hash_api_allocation_failures_report_enomem(hiplib):
    """The object's own device / pinned allocations made to fail (ablation build): HashBuffer returns ENOMEM, a stream's EndContext returns
    0 and latches ENOMEM; nothing aborts, and the same object works afterwards.  (lthip_blake2s_one and the lthip_b2s_stream pair
    allocate nothing: the caller's buffers are all they use.)"""
    from longtail_amd.lib import load_ablations

    abl = load_ablations()
    d = abl.dll
    p = d.Longtail_CreateHipBlake2HashAPI()
    assert p
    h = HashAPIStruct.from_address(p)
    data = np.random.default_rng(10).integers(0, 256, size=(3 << 20) + 5, dtype=np.uint8)
    out = C.c_uint64(0)
    assert h.HashBuffer(p, 100, data.ctypes.data, C.byref(out)) == 0 and out.value == b2(data[:100])  # the thread's context exists
    d.Longtail_Hip_GetLastError()
    try:
        assert d.lthip_debug_fail_alloc(0, 1 << 30) == 0
        assert h.HashBuffer(p, 3 << 20, data.ctypes.data, C.byref(out)) == errno.ENOMEM
        ctx = C.c_void_p()
        assert h.BeginContext(p, C.byref(ctx)) == 0
        h.Hash(p, ctx, len(data), data.ctypes.data)
        assert h.EndContext(p, ctx) == 0
        assert d.Longtail_Hip_GetLastError() == errno.ENOMEM
    finally:
        d.lthip_debug_fail_alloc(-1, 0)
    assert h.HashBuffer(p, 3 << 20, data.ctypes.data, C.byref(out)) == 0 and out.value == b2(data[: 3 << 20])
    ctx = C.c_void_p()
    assert h.BeginContext(p, C.byref(ctx)) == 0
    h.Hash(p, ctx, len(data), data.ctypes.data)
    assert h.EndContext(p, ctx) == b2(data)
    h.Dispose(p)
