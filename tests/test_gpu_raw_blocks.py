"""-m gpu: lthip_write_raw_block_images (include/longtail_hip.h) alone -- the complete image of blocks with tag 0, which the reference
stores as they are (CompressBlock, lib/compressblockstore/longtail_compressblockstore.c:85-90): BlockIndex + the chunks' bytes.

One call writes 48 blocks of 1, 2, 3, 4, 5 and 64 chunks (so the payload starts at every 4-byte phase of an 8-aligned image and later
chunks at every byte phase), chunk lengths around every size the copy treats differently (a byte-wise head or tail only, one 16-byte
vector, a 1 KiB wave round, a 4 KiB unrolled round, more than one 32 KiB piece), sources at every byte phase 0..15, blocks that are one
contiguous source run longer than a piece, blocks in runs of two chunks, and fully scattered blocks.  Against the reference (oracle/_ref,
through ctypes):

  * every image == Longtail_CreateStoredBlock(block hash, hash id, n, 0, hashes, sizes, raw) + payload copy +
    Longtail_WriteStoredBlockToBuffer, the block hash being Longtail_CreateBlockIndex's ('blk3'; for 'blk2' the oracle build has no
    BLAKE2 HashAPI, so the hash of the chunk-hash array, src/longtail.c:3753-3757, comes from hashlib.blake2s(digest_size=8))
  * Longtail_ReadStoredBlockFromBuffer opens every image with m_BlockChunksDataSize == raw
  * every arena byte outside the images is still the 0xA5 it was filled with

Every comparison is equality."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BLK3, BLK2 = 0x626C6B33, 0x626C6B32
LENGTHS = [1, 15, 16, 17, 47, 48, 63, 64, 65, 4095, 4096, 4097, 262143, 262145, (1 << 20) + 5]
COUNTS = [1, 2, 3, 4, 5, 64]


class RefBlockIndex(C.Structure):  # struct Longtail_BlockIndex (src/longtail.h)
    _fields_ = [("m_BlockHash", C.POINTER(C.c_uint64)), ("m_HashIdentifier", C.POINTER(C.c_uint32)), ("m_ChunkCount", C.POINTER(C.c_uint32)),
                ("m_Tag", C.POINTER(C.c_uint32)), ("m_ChunkHashes", C.c_void_p), ("m_ChunkSizes", C.c_void_p)]


class RefStoredBlock(C.Structure):  # struct Longtail_StoredBlock
    _fields_ = [("Dispose", C.CFUNCTYPE(None, C.c_void_p)), ("m_BlockIndex", C.POINTER(RefBlockIndex)), ("m_BlockData", C.c_void_p),
                ("m_BlockChunksDataSize", C.c_uint32)]


def _ref_calls(ref):
    d = ref.dll
    if not getattr(d, "_raw_block_sigs", False):
        d.Longtail_CreateBlake3HashAPI.restype = C.c_void_p
        d.Longtail_DisposeAPI.argtypes = [C.c_void_p]
        d.Longtail_Free.argtypes = [C.c_void_p]
        d.Longtail_CreateBlockIndex.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.POINTER(RefBlockIndex))]
        d.Longtail_CreateStoredBlock.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32,
                                                 C.POINTER(C.POINTER(RefStoredBlock))]
        d.Longtail_WriteStoredBlockToBuffer.argtypes = [C.POINTER(RefStoredBlock), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        d.Longtail_ReadStoredBlockFromBuffer.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(RefStoredBlock))]
        d._raw_block_sigs = True
    return d


def ref_block_hash(ref, hashes, sizes, hash_id=BLK3):
    """The block hash Longtail_CreateBlockIndex gives the chunks (tag 0)."""
    hashes, sizes = np.ascontiguousarray(hashes, np.uint64), np.ascontiguousarray(sizes, np.uint32)
    if hash_id == BLK2:
        return int.from_bytes(hashlib.blake2s(hashes.tobytes(), digest_size=8).digest(), "little")
    d = _ref_calls(ref)
    api = d.Longtail_CreateBlake3HashAPI()
    idx = np.arange(len(hashes), dtype=np.uint32)
    bi = C.POINTER(RefBlockIndex)()
    assert d.Longtail_CreateBlockIndex(api, 0, len(hashes), idx.ctypes.data, hashes.ctypes.data, sizes.ctypes.data, C.byref(bi)) == 0
    out = int(bi.contents.m_BlockHash[0])
    d.Longtail_Free(C.cast(bi, C.c_void_p))
    d.Longtail_DisposeAPI(api)
    return out


def ref_raw_image(ref, hashes, sizes, payload, hash_id=BLK3):
    """The reference's serialized stored block with tag 0 for these chunks: Longtail_CreateStoredBlock + the payload copied into
    m_BlockData + Longtail_WriteStoredBlockToBuffer."""
    d = _ref_calls(ref)
    hashes, sizes = np.ascontiguousarray(hashes, np.uint64).copy(), np.ascontiguousarray(sizes, np.uint32).copy()
    payload = np.ascontiguousarray(payload, np.uint8)
    raw = int(sizes.astype(np.int64).sum())
    assert raw == len(payload)
    sb = C.POINTER(RefStoredBlock)()
    assert d.Longtail_CreateStoredBlock(ref_block_hash(ref, hashes, sizes, hash_id), hash_id, len(hashes), 0, hashes.ctypes.data, sizes.ctypes.data,
                                        raw, C.byref(sb)) == 0
    if raw:
        C.memmove(sb.contents.m_BlockData, payload.ctypes.data, raw)
    buf, size = C.c_void_p(), C.c_size_t(0)
    assert d.Longtail_WriteStoredBlockToBuffer(sb, C.byref(buf), C.byref(size)) == 0
    out = np.frombuffer((C.c_ubyte * size.value).from_address(buf.value), np.uint8).copy()
    d.Longtail_Free(buf)
    sb.contents.Dispose(C.cast(sb, C.c_void_p))
    return out


def ref_opens_raw_image(ref, image):
    """Longtail_ReadStoredBlockFromBuffer -> m_BlockChunksDataSize (the image's bytes behind the BlockIndex)."""
    d = _ref_calls(ref)
    image = np.ascontiguousarray(image, np.uint8)
    sb = C.POINTER(RefStoredBlock)()
    assert d.Longtail_ReadStoredBlockFromBuffer(image.ctypes.data, len(image), C.byref(sb)) == 0
    size = int(sb.contents.m_BlockChunksDataSize)
    sb.contents.Dispose(C.cast(sb, C.c_void_p))
    return size


_case = {}


def the_case():
    """48 blocks over one source buffer -- made once, shared by the two hash types, never changed."""
    if _case:
        return _case
    rng = np.random.default_rng(2024)
    lens, offs, first = [], [], [3]  # (three chunks in front that belong to no block: block_first_chunk[0] != 0)
    pad_lens, pad_offs = [7, 7, 7], [0, 0, 0]
    cursor, phase, pick, long_runs, scattered = 64, 0, 0, 0, 0
    for b in range(48):
        n = COUNTS[b % 6]
        mode = (b // 6) % 3  # 0: one contiguous source run, 1: fully scattered, 2: runs of two chunks
        if n == 64:  # (64 chunks: keep the megabyte lengths out, the block stays below a few MiB)
            blens = [LENGTHS[(pick + i) % 12] for i in range(n)]
        else:
            blens = [LENGTHS[(pick + i) % len(LENGTHS)] for i in range(n)]
        if b == 0:
            blens = [(1 << 20) + 5]  # one chunk, one run of 33 pieces
        pick += 7
        for i, ln in enumerate(blens):
            joined = i > 0 and (mode == 0 or (mode == 2 and i % 2 == 1))
            if not joined:
                cursor = (cursor + 1 + 15) // 16 * 16 + phase  # at least one byte apart, every byte phase in turn
                phase = (phase + 1) % 16
            offs.append(cursor)
            lens.append(ln)
            cursor += ln
        raw = sum(blens)
        long_runs += mode == 0 and n > 1 and raw > (64 << 10)
        scattered += mode == 1 and n > 1
        first.append(first[-1] + n)
    assert long_runs >= 3 and scattered >= 5
    assert {o % 16 for o in offs} == set(range(16)) and set(lens) == set(LENGTHS)
    src = rng.integers(0, 256, size=cursor, dtype=np.uint8)  # (the last chunk ends at the buffer's last byte)
    lens_all = np.array(pad_lens + lens, np.uint32)
    offs_all = np.array(pad_offs + offs, np.uint64)
    hashes = rng.integers(1, 2**63, size=len(lens_all), dtype=np.uint64)
    first = np.array(first, np.uint64)
    # images: 8-aligned, some back to back, some with a gap
    image_offs, at = [], 40
    for b in range(48):
        n = int(first[b + 1] - first[b])
        raw = int(lens_all[int(first[b]) : int(first[b + 1])].astype(np.int64).sum())
        at = (at + [0, 8, 24, 200][b % 4] + 7) // 8 * 8
        image_offs.append(at)
        at += 20 + 12 * n + raw
    payload_phases = {(o + 20 + 12 * int(first[b + 1] - first[b])) % 16 for b, o in enumerate(image_offs)}
    assert payload_phases == {0, 4, 8, 12}
    _case.update(src=src, lens=lens_all, offs=offs_all, hashes=hashes, first=first, image_offs=np.array(image_offs, np.uint64), arena_bytes=at + 333)
    return _case


@pytest.mark.parametrize("hash_id", [BLK3, BLK2], ids=["blk3", "blk2"])
def test_raw_block_images_are_the_references_bytes(gpu, ref, hash_id):
    c = the_case()
    d = gpu.lib.dll
    for n in (0, 1, 64):
        assert gpu.block_index_size(n) == 20 + 12 * n == int(d.lthip_stored_block_header_size(n)) - 8
    src = torch.from_numpy(c["src"]).cuda()
    d_len = torch.from_numpy(c["lens"].view(np.int32)).cuda()
    d_off = torch.from_numpy(c["offs"].view(np.int64)).cuda()
    d_hash = torch.from_numpy(c["hashes"].view(np.int64)).cuda()
    arena = torch.full((c["arena_bytes"],), 0xA5, dtype=torch.uint8, device="cuda")
    gpu.write_raw_block_images(c["first"], d_hash, d_len, d_off, src, arena, c["image_offs"], hash_identifier=hash_id)
    gpu.sync()
    host = arena.cpu().numpy()
    untouched = np.ones(len(host), bool)
    for b, at in enumerate(c["image_offs"].tolist()):
        c0, c1 = int(c["first"][b]), int(c["first"][b + 1])
        h, s = c["hashes"][c0:c1], c["lens"][c0:c1]
        payload = np.concatenate([c["src"][int(o) : int(o) + int(n)] for o, n in zip(c["offs"][c0:c1], s)])
        expect = ref_raw_image(ref, h, s, payload, hash_id)
        assert len(expect) == gpu.block_index_size(c1 - c0) + len(payload)
        got = host[at : at + len(expect)]
        assert int(np.frombuffer(got[:8].tobytes(), np.uint64)[0]) == ref_block_hash(ref, h, s, hash_id), b
        assert (got == expect).all(), (b, c1 - c0, int(np.flatnonzero(got != expect)[0]))
        assert ref_opens_raw_image(ref, got) == len(payload), b
        untouched[at : at + len(expect)] = False
    assert (host[untouched] == 0xA5).all(), "a byte outside the images was written"
    assert untouched.sum() > 333


def test_no_blocks_and_bad_tables(gpu):
    d = gpu.lib.dll
    assert d.lthip_write_raw_block_images(gpu.h, 0, None, None, None, None, None, BLK3, None, None) == 0
    assert d.lthip_write_raw_block_images(None, 0, None, None, None, None, None, BLK3, None, None) != 0
    t = torch.zeros(64, dtype=torch.int64, device="cuda")
    first, off = np.array([0, 1], np.uint64), np.array([4], np.uint64)  # an image offset that is not 8-byte aligned
    import errno

    assert d.lthip_write_raw_block_images(gpu.h, 1, first.ctypes.data, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), BLK3, t.data_ptr(),
                                          off.ctypes.data) == errno.EINVAL
