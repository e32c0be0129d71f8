"""-m gpu: the 'meow' hash type (Meow hash v0.5, low 64 bits, lib/meowhash/longtail_meowhash.c) against the reference's own digests
(tests/golden/meow_vectors.json) and the project's CPU model (tests/meow_model.py), and, through the reference core (oracle/_ref) with a
model-backed Python HashAPI, the VersionIndex / StoreIndex a 'meow' store holds:

  * lthip_meow_ranges[_dev], _one, _runs_u64, the streaming pair: every golden length, any start offset, many mixed ranges, long ones
    among many, the device count behind lthip_chunk_hash(d_chunk_hashes = NULL)
  * Longtail_CreateHipMeowHashAPI: identifier 'meow', the five entry points, found by Longtail_CreateDefaultHashRegistry next to the
    BLAKE3 and BLAKE2 objects; one chunker window looked up by the BLAKE2 and the Meow object gives each its own digests
  * Longtail_CreateVersionIndex with HIP chunker + HIP Meow and with the reference chunker + HIP Meow == with the model HashAPI
  * the bulk session with hash_identifier 'meow': VersionIndex, StoreIndex and stored-block headers
  * injected allocation failures give ENOMEM, and the next call works"""
import ctypes as C
import errno
import hashlib
import threading

import numpy as np
import pytest
import torch

from longtail_amd.dist import JobPartition
from longtail_amd.lib import HASH_BLAKE2, HASH_BLAKE3, HASH_MEOW, Context, Ingest, chunker_params
from tests.gpu_util import dev_u32, dev_u64, to_device, u32, u64
from tests.meow_model import meow, meow_batch
from tests.test_gpu_ingest import parse_store_index, ref_missing_content, version_unique_lists
from tests.test_gpu_plugins import ChunkerAPIStruct, HashAPIStruct, PyHashAPI
from tests.test_meow_abi import GOLDEN, golden_input

pytestmark = pytest.mark.gpu
M = 1 << 20


def model_ranges(host, offs, lens) -> np.ndarray:
    """the model's digests of host[o : o + n], hashed in groups of similar length"""
    offs, lens = np.asarray(offs, np.int64), np.asarray(lens, np.int64)
    out = np.zeros(len(lens), np.uint64)
    order = np.argsort(lens, kind="stable")
    for g in range(0, len(order), 2048):
        idx = order[g : g + 2048]
        w = max(1, int(lens[idx].max()))
        m = np.zeros((len(idx), w), np.uint8)
        for r, i in enumerate(idx):
            m[r, : lens[i]] = host[offs[i] : offs[i] + lens[i]]
        out[idx] = meow_batch(m, lens[idx])
    return out


@pytest.fixture(scope="module")
def gpu():
    ctx = Context(0)
    yield ctx
    ctx.close()


def check_ranges(gpu, host, offs, lens, max_len=0, expect=None):
    dev = torch.from_numpy(host).cuda()
    got = u64(gpu.meow_ranges(dev, dev_u64(offs), dev_u32(lens), max_len))
    exp = model_ranges(host, offs, lens) if expect is None else np.asarray(expect, np.uint64)
    bad = np.nonzero(got[: len(exp)] != exp)[0]
    assert len(bad) == 0, [(int(offs[i]), int(lens[i])) for i in bad[:8]]


def golden_host():
    """every golden vector's input in one buffer (16-byte aligned starts + their own offset residue), with offsets and digests"""
    vs = GOLDEN["vectors"]
    pos, offs, parts = 0, [], []
    for v in vs:
        d = golden_input(v)
        start = pos + (v["offset"] % 16)
        offs.append(start)
        parts.append((start, d))
        pos = (start + len(d) + 16 + 15) // 16 * 16
    host = np.zeros(pos + 64, np.uint8)
    for start, d in parts:
        host[start : start + len(d)] = d
    return host, offs, [v["len"] for v in vs], [int(v["digest"], 16) for v in vs]


def test_ranges_golden_digests(gpu):
    host, offs, lens, digests = golden_host()
    check_ranges(gpu, host, offs, lens, expect=digests)  # few ranges: the quad kernel
    k = 12  # > 256 ranges: the length-class order, long ranges on quads, the rest one lane per range
    check_ranges(gpu, host, offs * k, lens * k, max(lens), expect=digests * k)


def test_ranges_lengths_and_offsets(gpu):
    rng = np.random.default_rng(2)
    host = rng.integers(0, 256, size=(1 << 20) + 64, dtype=np.uint8)
    special = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 127, 128, 255, 256, 257, 511, 512, 1023, 4095, 4096, 4097]
    offs, lens = [], []
    for n in special:
        for r in range(16):  # every start residue mod 16
            offs.append(1000 + 16 * int(rng.integers(0, 100)) + r)
            lens.append(n)
    exp = model_ranges(host, offs, lens)
    check_ranges(gpu, host, offs, lens, expect=exp)
    check_ranges(gpu, host, offs * 3, lens * 3, 4097, expect=np.tile(exp, 3))
    for count in (1, 2, 257):
        o = rng.integers(0, 700000, size=count)
        n = rng.integers(0, 40000, size=count)
        check_ranges(gpu, host, o, n)


def test_ranges_many(gpu):
    rng = np.random.default_rng(3)
    host = rng.integers(0, 256, size=(4 << 20) + 64, dtype=np.uint8)
    count = 40000
    o = rng.integers(0, 4 << 20, size=count)
    n = np.minimum(rng.integers(0, 3000, size=count), (4 << 20) - o)
    n[::997] = 0
    check_ranges(gpu, host, o, n)


def test_ranges_long_ones_among_many(gpu):
    rng = np.random.default_rng(8)
    host = rng.integers(0, 256, size=(6 << 20) + 64, dtype=np.uint8)
    o = list(rng.integers(0, 1 << 20, size=400))
    n = list(rng.integers(0, 5000, size=400))
    for k, (off, ln) in enumerate([(3, 2 * M + 5), (17, M - 1), (64, M), (5, M + 255), (1000, 3 * M)]):
        o.insert(37 * k, off)
        n.insert(37 * k, ln)
    check_ranges(gpu, host, o, n)
    first = np.array([0, 1 << 17, (1 << 17) + 3] + [(1 << 17) + 3 + 10 * k for k in range(1, 300)], np.uint32)
    vals = host[: 8 * int(first[-1])].view(np.uint64)
    got = u64(gpu.meow_runs_u64(dev_u64(vals), dev_u32(first), len(first) - 1))
    assert list(got) == [meow(vals[first[i] : first[i + 1]].tobytes()) for i in range(len(first) - 1)]
    assert gpu.lib.dll.lthip_meow_runs_u64(gpu.h, dev_u64(vals).data_ptr(), dev_u32(first).data_ptr(), 0, dev_u64(vals).data_ptr()) == 0


@pytest.mark.parametrize("source", ["golden", "synth"])
def test_ranges_device_count_behind_the_chunker(gpu, golden, oracle, source):
    if source == "golden":
        data, target = golden["chunker_input"], 4096
    else:
        data, target = oracle.synth(8 << 20, 11, 1), 65536
    mn, av, mx = chunker_params(target)
    dev, offs = to_device([data])
    plan = gpu.make_plan(offs, [len(data)], mn, av, mx)
    total, d_off, d_len, d_hash, d_first = gpu.chunk_hash(plan, dev, want_hashes=False, sync=False)
    cap = plan.capacity
    out = torch.full((cap,), -1, dtype=torch.int64, device="cuda")
    gpu.meow_ranges(dev, d_off, d_len, mx, out=out, count_bound=cap, d_count=d_first[1:])
    n = int(u32(d_first)[1])
    got = u64(out)
    ho, hl = u64(d_off)[:n], u32(d_len)[:n]
    assert (got[:n] == model_ranges(data, ho, hl)).all()
    assert (got[n:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), "slots beyond the device count were written"
    plan.close()


def test_one_any_alignment(gpu):
    src = np.random.default_rng(9).integers(0, 256, size=65536 + 64, dtype=np.uint8)
    pin = torch.from_numpy(src.copy()).pin_memory()
    out = torch.zeros(1, dtype=torch.int64).pin_memory()
    for start in (0, 1, 2, 3, 5, 15):
        for n in (0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1000, 4096, 65536 - 16, 65536):
            gpu.meow_one(pin[start:], n, out)
            gpu.sync()
            assert int(out.numpy().view(np.uint64)[0]) == meow(src[start : start + n]), (start, n)
    dev = torch.from_numpy(src.copy()).cuda()
    dout = torch.zeros(1, dtype=torch.int64, device="cuda")
    for n in (0, 100, 65536):
        gpu.meow_one(dev, n, dout)
        assert int(u64(dout)[0]) == meow(src[:n]), n
    assert gpu.lib.dll.lthip_meow_one(gpu.h, pin.data_ptr(), 65537, out.data_ptr()) == errno.EINVAL


def test_stream(gpu):
    host, offs, lens, digests = golden_host()
    dev = torch.from_numpy(host).cuda()
    for o, n, d in zip(offs, lens, digests):
        if o % 16 == 0:  # the stream's batches are 16-byte aligned device memory
            assert gpu.meow_stream(dev[o:], n) == d, n
    rng = np.random.default_rng(6)
    h = rng.integers(0, 256, size=3 * M + 64, dtype=np.uint8)
    d = torch.from_numpy(h).cuda()
    for n in (M - 1, M, M + 1, 2 * M + 255, 3 * M):
        assert gpu.meow_stream(d, n) == meow(h[:n]), n


# ---- the HashAPI object ----
@pytest.fixture(scope="module")
def hip_meow(hiplib):
    p = hiplib.dll.Longtail_CreateHipMeowHashAPI()
    assert p
    yield p
    HashAPIStruct.from_address(p).Dispose(p)


def test_hash_api_entry_points(hip_meow):
    h = HashAPIStruct.from_address(hip_meow)
    assert h.GetIdentifier(hip_meow) == HASH_MEOW == 0x6D656F77
    out = C.c_uint64(0)
    assert h.HashBuffer(hip_meow, 0, b"\0", C.byref(out)) == 0 and out.value == meow(b"")
    st = GOLDEN["stream"]
    data = np.ascontiguousarray(golden_input(st))
    for n in (1, 255, 256, 257, 65536, 70000, M + 3):
        assert h.HashBuffer(hip_meow, n, data.ctypes.data, C.byref(out)) == 0
        assert out.value == meow(data[:n]), n
    full = int(st["digest"], 16)
    golden_cuts = list(np.cumsum(st["pieces"]))
    for cuts in (golden_cuts, [], [0], [1], [255, 256, 257], [1000, 150000], [M - 1, M + 1], [M], [5, len(data) - 1]):
        ctx = C.c_void_p()
        assert h.BeginContext(hip_meow, C.byref(ctx)) == 0
        pts = [0] + [int(c) for c in cuts] + [len(data)]
        for a, b in zip(pts, pts[1:]):
            h.Hash(hip_meow, ctx, b - a, data.ctypes.data + a)
        assert h.EndContext(hip_meow, ctx) == full, cuts
    ctx = C.c_void_p()
    assert h.BeginContext(hip_meow, C.byref(ctx)) == 0
    assert h.EndContext(hip_meow, ctx) == meow(b"")


# a Longtail_HashAPI backed by the CPU model: the reference core with it builds the reference's 'meow' VersionIndex
@pytest.fixture(scope="module")
def py_meow():
    return PyHashAPI(HASH_MEOW, meow)


def small_files(oracle):
    """a tree of a few MiB: the reference core calls the model once per chunk"""
    rng = np.random.default_rng(77)
    files = [(f"d{i % 2}/f{i:02d}.bin", oracle.synth(int(rng.integers(1, 400000)), 90 + i, i % 3)) for i in range(6)]
    files.append(("d0/copy.bin", files[2][1].copy()))
    files.append(("empty.bin", np.zeros(0, np.uint8)))
    files.append(("zeros.bin", np.zeros(100000, np.uint8)))
    return files


@pytest.mark.parametrize("workers", [0, 4])
def test_reference_version_index_with_hip_meow(ref, oracle, hiplib, hip_meow, py_meow, workers):
    files = small_files(oracle)
    expect, _ = ref.version_index(files, 4096, workers, ref.lz4_type, hash_api=py_meow.ptr)
    assert np.frombuffer(expect[:8], np.uint32)[1] == HASH_MEOW
    got_ref_chunker, _ = ref.version_index(files, 4096, workers, ref.lz4_type, hash_api=hip_meow)
    assert got_ref_chunker == expect
    chunker = hiplib.dll.Longtail_CreateHipChunkerAPI()
    try:
        got_hip, _ = ref.version_index(files, 4096, workers, ref.lz4_type, chunker_api=chunker, hash_api=hip_meow)
    finally:
        ChunkerAPIStruct.from_address(chunker).Dispose(chunker)
    assert got_hip == expect


def test_hash_registry_returns_each_hip_object(ref, hiplib):
    d = ref.dll
    d.Longtail_CreateDefaultHashRegistry.restype = C.c_void_p
    d.Longtail_CreateDefaultHashRegistry.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    d.Longtail_GetHashRegistry_GetHashAPI.restype = C.c_int
    d.Longtail_GetHashRegistry_GetHashAPI.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    objs = {HASH_BLAKE3: hiplib.dll.Longtail_CreateHipBlake3HashAPI(), HASH_BLAKE2: hiplib.dll.Longtail_CreateHipBlake2HashAPI(),
            HASH_MEOW: hiplib.dll.Longtail_CreateHipMeowHashAPI()}
    types = (C.c_uint32 * 3)(*objs.keys())
    apis = (C.c_void_p * 3)(*objs.values())
    reg = d.Longtail_CreateDefaultHashRegistry(3, types, apis)
    assert reg
    for t, p in objs.items():
        out = C.c_void_p()
        assert d.Longtail_GetHashRegistry_GetHashAPI(reg, t, C.byref(out)) == 0 and out.value == p
        assert HashAPIStruct.from_address(out.value).GetIdentifier(out.value) == t
    HashAPIStruct.from_address(reg).Dispose(reg)  # (a Longtail_API first, like every longtail object)


def test_one_window_serves_blake2_and_meow(ref, oracle, hiplib, hip_meow, py_meow):
    """Longtail_CreateVersionIndex with the HIP chunker and a Python HashAPI whose HashBuffer asks the HIP BLAKE2 object, the HIP Meow
    object and the BLAKE2 object again for each chunk of the chunker's window: each gets its own kind's digests."""
    b2 = hiplib.dll.Longtail_CreateHipBlake2HashAPI()
    h2, hm = HashAPIStruct.from_address(b2), HashAPIStruct.from_address(hip_meow)
    bad, calls = [], []

    def buffer(api, length, data, out):
        chunk = C.string_at(data, length) if length else b""
        o2, om, o2b = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        e = (h2.HashBuffer(b2, length, data, C.byref(o2)), hm.HashBuffer(hip_meow, length, data, C.byref(om)),
             h2.HashBuffer(b2, length, data, C.byref(o2b)))
        want2 = int.from_bytes(hashlib.blake2s(chunk, digest_size=8).digest(), "little")
        wantm = meow(chunk)
        calls.append(length)
        if e != (0, 0, 0) or o2.value != want2 or o2b.value != want2 or om.value != wantm:
            bad.append((length, e))
        out[0] = wantm
        return 0

    f = dict(HashAPIStruct._fields_)
    cbs = [f["Dispose"](lambda api: None), f["GetIdentifier"](lambda api: HASH_MEOW), f["BeginContext"](py_meow._begin),
           f["Hash"](py_meow._hash), f["EndContext"](py_meow._end), f["HashBuffer"](buffer)]
    both = HashAPIStruct(*cbs)
    files = small_files(oracle)
    chunker = hiplib.dll.Longtail_CreateHipChunkerAPI()
    try:
        got, _ = ref.version_index(files, 4096, 0, ref.lz4_type, chunker_api=chunker, hash_api=C.addressof(both))
    finally:
        ChunkerAPIStruct.from_address(chunker).Dispose(chunker)
        h2.Dispose(b2)
    assert len(calls) > 50 and not bad, bad[:8]
    assert got == ref.version_index(files, 4096, 0, ref.lz4_type, hash_api=py_meow.ptr)[0]


# ---- the bulk session with hash_identifier 'meow' ----
def meow_session(gpu, ref, files, target, max_block, max_chunks, tag):
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
    total, d_off, d_len, _, d_first = gpu.chunk_hash(plan, dev, want_hashes=False)
    d_hash = torch.empty(max(1, plan.capacity), dtype=torch.int64, device="cuda")
    gpu.meow_ranges(dev, d_off, d_len, mx, out=d_hash, count_bound=plan.capacity, d_count=d_first[plan.nparts:])
    plan.close()
    job_first = u32(d_first).astype(np.uint64)
    ing = Ingest(gpu, target, max_block, max_chunks, "lz4", compression_type=tag, hash_identifier=HASH_MEOW)
    tree, keep = Ingest.tree(sizes.copy(), offs.copy(), perms.copy(), path_data, part.job_asset.copy(), job_first.copy())
    vi = torch.zeros(gpu.lib.dll.lthip_version_index_size(len(sizes), total, total, len(path_data)) + 64, dtype=torch.uint8).pin_memory()
    ing.index(tree, d_hash[:total], d_len[:total], total, d_off, d_first, total, vi)
    arena = torch.zeros(32 << 20, dtype=torch.uint8, device="cuda")
    ing.write(dev, arena)
    si = torch.zeros(16 + 32 * max(total, 1) + 64, dtype=torch.uint8).pin_memory()
    res = ing.finish(si)
    return dict(vi=bytes(vi.numpy()[: res.version_index_size]), si=bytes(si.numpy()[: res.store_index_size]), res=res, ing=ing, arena=arena)


def test_ingest_session_meow_matches_reference(gpu, oracle, ref, py_meow):
    files = small_files(oracle)
    target, max_block, max_chunks, tag = 4096, 65536, 16, ref.lz4_type
    sess = meow_session(gpu, ref, files, target, max_block, max_chunks, tag)
    expect_vi, _ = ref.version_index(files, target, 0, tag, hash_api=py_meow.ptr)
    assert sess["vi"] == expect_vi, "Meow VersionIndex differs from Longtail_CreateVersionIndex with a Meow HashAPI"
    uh, us, ut = version_unique_lists(expect_vi)
    si = bytearray(ref_missing_content(ref, np.zeros(0, np.uint64), uh, us, ut, max_block, max_chunks))
    np.frombuffer(si, np.uint32, 1, 4)[:] = HASH_MEOW
    p = parse_store_index(bytes(si))
    starts = np.concatenate([[0], np.cumsum(p["block_counts"])]).astype(np.int64)
    for b in range(len(p["block_hashes"])):  # src/longtail.c:3757: the block hash is the hash of the block's chunk hashes
        np.frombuffer(si, np.uint64, 1, 16 + 8 * b)[:] = meow(p["chunk_hashes"][starts[b] : starts[b + 1]].tobytes())
    assert sess["si"] == bytes(si)
    # every stored-block image's BlockIndex header: the Meow block hash, 'meow', the chunk count and the tag
    got = parse_store_index(sess["si"])
    _, offs, sizes = sess["ing"].images()
    arena = sess["arena"].cpu().numpy()
    assert len(offs) == sess["res"].blocks > 0
    for b in range(len(offs)):
        c0, n = int(got["block_offsets"][b]), int(got["block_counts"][b])
        head = np.frombuffer(arena[int(offs[b]) : int(offs[b]) + 20].tobytes(), np.uint32)
        assert int(head[0]) | (int(head[1]) << 32) == meow(np.ascontiguousarray(got["chunk_hashes"][c0 : c0 + n]).tobytes())
        assert head[2] == HASH_MEOW and head[3] == n and head[4] == tag, b
    sess["ing"].close()


def test_meow_allocation_failures_report_enomem(hiplib):
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
        err = d.lthip_meow_ranges(ctx.h, data.data_ptr(), n, offs.data_ptr(), lens.data_ptr(), 0, out.data_ptr())
        assert err == errno.ENOMEM, err
    finally:
        d.lthip_debug_fail_alloc(-1, 0)
    assert d.lthip_meow_ranges(ctx.h, data.data_ptr(), n, offs.data_ptr(), lens.data_ptr(), 0, out.data_ptr()) == 0
    ctx.sync()
    host = data.cpu().numpy()
    assert int(u64(out)[7]) == meow(host[700:800])
    ctx.close()

    # the object's part runs on a thread of its own: the per-thread buffers it grows are not the calling thread's, which later
    # tests of other objects find as they left them
    errors = []

    def object_failures():
        try:
            _object_failures(d)
        except BaseException as e:  # noqa: BLE001 (re-raised below)
            errors.append(e)

    t = threading.Thread(target=object_failures)
    t.start()
    t.join()
    if errors:
        raise errors[0]


def _object_failures(d):
    p = d.Longtail_CreateHipMeowHashAPI()
    assert p
    h = HashAPIStruct.from_address(p)
    big = np.random.default_rng(10).integers(0, 256, size=(3 << 20) + 5, dtype=np.uint8)
    o = C.c_uint64(0)
    assert h.HashBuffer(p, 100, big.ctypes.data, C.byref(o)) == 0 and o.value == meow(big[:100])
    d.Longtail_Hip_GetLastError()
    try:
        assert d.lthip_debug_fail_alloc(0, 1 << 30) == 0
        assert h.HashBuffer(p, 3 << 20, big.ctypes.data, C.byref(o)) == errno.ENOMEM
        c = C.c_void_p()
        assert h.BeginContext(p, C.byref(c)) == 0
        h.Hash(p, c, len(big), big.ctypes.data)
        assert h.EndContext(p, c) == 0
        assert d.Longtail_Hip_GetLastError() == errno.ENOMEM
    finally:
        d.lthip_debug_fail_alloc(-1, 0)
    assert h.HashBuffer(p, 3 << 20, big.ctypes.data, C.byref(o)) == 0 and o.value == meow(big[: 3 << 20])
    c = C.c_void_p()
    assert h.BeginContext(p, C.byref(c)) == 0
    h.Hash(p, c, len(big), big.ctypes.data)
    assert h.EndContext(p, c) == meow(big)
    h.Dispose(p)
