"""Helpers of the archive tests: the reference's archive index through ctypes (Longtail_CreateArchiveIndex / Longtail_ReadArchiveIndex of
oracle/_ref/liblongtail_ref.so, src/longtail.c:9921-10090), a Python reading of the same layout, and a small hand-built store whose blocks
have 1, 64, 65 and 130 chunks, raw and LZ4-tagged (the tagged payloads are LZ4 blocks of literals only, written here)."""
import ctypes as C

import numpy as np

from tests.restore_util import BLK3, block_index_bytes, build_store_index, build_version_index, parse_store_index, raw_image

LZ4 = 0x6C7A3432  # 'lz42'
ARCHIVE_VERSION = 1


class RefArchive:
    """struct Longtail_ArchiveIndex (src/longtail.h:1883-1891) is pointers into one allocation: m_Version, m_IndexDataSize, the ten
    pointers of the StoreIndex, m_BlockStartOffets, m_BlockSizes, then the VersionIndex (first m_Version)."""

    def __init__(self, ref):
        d = self.d = ref.dll
        vp = C.c_void_p
        for name, res, args in (("Longtail_ReadStoreIndexFromBuffer", C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
                                ("Longtail_ReadVersionIndexFromBuffer", C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
                                ("Longtail_CreateArchiveIndex", C.c_int, [vp, vp, C.POINTER(vp)]),
                                ("Longtail_ReadArchiveIndex", C.c_int, [vp, C.c_char_p, C.POINTER(vp)]),
                                ("Longtail_CreateFSStorageAPI", vp, []), ("Longtail_Free", None, [vp]), ("Longtail_DisposeAPI", None, [vp])):
            f = getattr(d, name)
            f.restype, f.argtypes = res, args

    @staticmethod
    def _fields(ai):
        w = (C.c_uint64 * 15).from_address(ai)
        size = C.c_uint32.from_address(w[1]).value
        return dict(data=w[0], size=size, offsets=w[12], sizes=w[13], vi_at=w[14] - w[0])

    def create(self, si: bytes, vi: bytes, offsets, sizes):
        """-> the bytes behind Longtail_CreateArchiveIndex with these offsets and sizes stored into its tables, or the errno."""
        psi, pvi, ai = C.c_void_p(), C.c_void_p(), C.c_void_p()
        bsi, bvi = np.frombuffer(si, np.uint8).copy(), np.frombuffer(vi, np.uint8).copy()
        err = self.d.Longtail_ReadStoreIndexFromBuffer(bsi.ctypes.data, len(bsi), C.byref(psi))
        if err:
            return err
        err = self.d.Longtail_ReadVersionIndexFromBuffer(bvi.ctypes.data, len(bvi), C.byref(pvi))
        assert err == 0, err
        err = self.d.Longtail_CreateArchiveIndex(psi, pvi, C.byref(ai))
        try:
            if err:
                return err
            f = self._fields(ai.value)
            o, z = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(sizes, np.uint32)
            if len(o):
                C.memmove(f["offsets"], o.ctypes.data, o.nbytes)
                C.memmove(f["sizes"], z.ctypes.data, z.nbytes)
            return C.string_at(f["data"], f["size"])
        finally:
            for p in (ai, pvi, psi):
                if p.value:
                    self.d.Longtail_Free(p)

    def read(self, path: str):
        """Longtail_ReadArchiveIndex over the FS storage API -> dict(index bytes, offsets, sizes, vi_at), or the errno."""
        fs, ai = self.d.Longtail_CreateFSStorageAPI(), C.c_void_p()
        try:
            err = self.d.Longtail_ReadArchiveIndex(fs, path.encode(), C.byref(ai))
            if err:
                return err
            f = self._fields(ai.value)
            index = C.string_at(f["data"], f["size"])
            nb = int(np.frombuffer(index[16:20], np.uint32)[0])
            out = dict(index=index, vi_at=int(f["vi_at"]),
                       offsets=np.frombuffer(C.string_at(f["offsets"], 8 * nb), np.uint64).copy(),
                       sizes=np.frombuffer(C.string_at(f["sizes"], 4 * nb), np.uint32).copy())
            self.d.Longtail_Free(ai)
            return out
        finally:
            self.d.Longtail_DisposeAPI(fs)


def parts_of_index(index: bytes):
    """The archive index read in Python: dict(version, stored size, si, offsets, sizes, vi = the rest of the index)."""
    version, stored, _, _, nb, m = (int(x) for x in np.frombuffer(index[:24], np.uint32))
    s = 16 + 20 * nb + 12 * m
    at = 8 + s
    offsets = np.frombuffer(index[at : at + 8 * nb], np.uint64).copy()
    sizes = np.frombuffer(index[at + 8 * nb : at + 12 * nb], np.uint32).copy()
    return dict(version=version, stored=stored, si=index[8:at], tables_at=at, offsets=offsets, sizes=sizes, vi_at=at + 12 * nb,
                vi=index[at + 12 * nb :])


def lz4_literals(content: bytes) -> bytes:
    """An LZ4 block that is one run of literals (the last sequence of a block has no match)."""
    n = len(content)
    if n < 15:
        return bytes([n << 4]) + content
    ext, rest = b"", n - 15
    while rest >= 255:
        ext, rest = ext + b"\xff", rest - 255
    return b"\xf0" + ext + bytes([rest]) + content


def tagged_image(block_hash, hash_id, tag, chunk_hashes, chunk_sizes, payload: bytes, raw: int):
    words = np.array([raw, len(payload)], np.uint32).tobytes()
    return np.frombuffer(block_index_bytes(block_hash, hash_id, tag, chunk_hashes, chunk_sizes) + words + payload, np.uint8).copy()


def header_bytes(n, tag):
    return 20 + 12 * n + (8 if tag else 0)


COUNTS = (1, 64, 65, 130)  # the check's lane loop ends in its first round, fills it, wraps, wraps twice


def hand_store(oracle, seed=5, counts=COUNTS):
    """Blocks of `counts` chunks, each once raw and once LZ4-tagged; one asset per block (its chunks in order) and one asset that takes
    a chunk of every block.  -> dict(vi, si, images, block_hashes, tags, files (per asset), names)."""
    rng = np.random.default_rng(seed)
    lens, blocks, at = [], [], 0
    for k, n in enumerate(counts):
        for tag in (0, LZ4):
            blocks.append((0xB10C0000 + 16 * k + (1 if tag else 0), tag, list(range(at, at + n))))
            lens += [int(x) for x in rng.integers(1, 41, n)]
            at += n
    content = rng.integers(0, 256, sum(lens)).astype(np.uint8)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    hashes = oracle.blake3_many(content, starts, lens)
    assert len(set(int(h) for h in hashes)) == len(hashes)
    piece = lambda c: content[int(starts[c]) : int(starts[c]) + lens[c]]
    images = []
    for bh, tag, cs in blocks:
        body = np.concatenate([piece(c) for c in cs]).tobytes()
        h, s = hashes[cs], np.array(lens, np.uint32)[cs]
        images.append(raw_image(bh, BLK3, h, s, body) if not tag else tagged_image(bh, BLK3, tag, h, s, lz4_literals(body), len(body)))
    asset_chunks = [cs for _, _, cs in blocks] + [[cs[-1] for _, _, cs in blocks]]
    names = [f"block{b}.bin" for b in range(len(blocks))] + ["mixed.bin"]
    vi = build_version_index(BLK3, 32768, names, asset_chunks, hashes, lens)
    si = build_store_index(BLK3, blocks, hashes, lens)
    files = [np.concatenate([piece(c) for c in cs]) for cs in asset_chunks]
    chunk_block = [b for b, (_, _, cs) in enumerate(blocks) for _ in cs]
    return dict(vi=vi, si=si, images=images, block_hashes=parse_store_index(si)["block_hashes"], tags=[t for _, t, _ in blocks], files=files,
                names=names, counts=[len(cs) for _, _, cs in blocks], asset_chunks=asset_chunks, lens=lens, chunk_block=chunk_block,
                chunks=[piece(c) for c in range(len(lens))], blocks=blocks, hashes=hashes)


def expected_output(st, offsets, out_bytes, good_blocks=None, fill=0xA5):
    """What a restore of hand_store's version writes at these asset offsets when only `good_blocks` (default: all) are good."""
    out = np.full(out_bytes, fill, np.uint8)
    for cs, off in zip(st["asset_chunks"], offsets):
        at = int(off)
        for c in cs:
            if good_blocks is None or st["chunk_block"][c] in good_blocks:
                out[at : at + st["lens"][c]] = st["chunks"][c]
            at += st["lens"][c]
    return out


def place(images, offsets, body_bytes=None, fill=0x5A):
    """The images at these body offsets -> the body as a numpy array (exactly as long as its last image ends, or body_bytes)."""
    end = max([int(o) + len(i) for o, i in zip(offsets, images)], default=0)
    body = np.full(end if body_bytes is None else body_bytes, fill, np.uint8)
    for o, i in zip(offsets, images):
        body[int(o) : int(o) + len(i)] = i
    return body


def offsets_at_residue(images, residue, mod=8, order=None, gap=0):
    """Body offsets that put every image at `residue` mod `mod`, in `order` (default: as listed), at least `gap` bytes apart."""
    order = list(range(len(images))) if order is None else order
    offs, at = [0] * len(images), 0
    for b in order:
        at += gap
        at += (residue - at) % mod
        offs[b] = at
        at += len(images[b])
    return np.array(offs, np.uint64)
