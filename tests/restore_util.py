"""Helpers of the restore tests: serialized VersionIndex / StoreIndex blobs and stored-block images built in Python, layout for layout what
the library's writers and the reference produce (VersionIndex src/longtail.c:2551-2584, StoreIndex :8913-8931, stored block :4111-4150),
and readers for the same."""
import numpy as np

BLK3, BLK2, MEOW = 0x626C6B33, 0x626C6B32, 0x6D656F77
VERSION_INDEX_VERSION, STORE_INDEX_VERSION = 2, 1 << 24


def build_version_index(hash_id, target, names, asset_chunks, chunk_hashes, chunk_sizes, chunk_tags=None):
    """names[a]: the asset's path (a directory ends with '/'); asset_chunks[a]: indices into the unique chunk lists."""
    na, nu = len(names), len(chunk_hashes)
    chunk_sizes = np.asarray(chunk_sizes, np.uint32)
    counts = np.array([len(c) for c in asset_chunks], np.uint32)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32) if na else np.zeros(0, np.uint32)
    idx = np.array([c for cs in asset_chunks for c in cs], np.uint32)
    sizes = np.array([int(chunk_sizes[list(cs)].astype(np.int64).sum()) if len(cs) else 0 for cs in asset_chunks], np.uint64)
    name_data = b"".join(n.encode() + b"\0" for n in names)
    name_offs = np.array([sum(len(n.encode()) + 1 for n in names[:a]) for a in range(na)], np.uint32)
    head = np.array([VERSION_INDEX_VERSION, hash_id, target, na, nu, len(idx)], np.uint32)
    tags = np.zeros(nu, np.uint32) if chunk_tags is None else np.asarray(chunk_tags, np.uint32)
    return b"".join([head.tobytes(), np.arange(1, na + 1, dtype=np.uint64).tobytes(), np.arange(101, na + 101, dtype=np.uint64).tobytes(),
                     sizes.tobytes(), counts.tobytes(), starts.tobytes(), idx.tobytes(), np.asarray(chunk_hashes, np.uint64).tobytes(),
                     chunk_sizes.tobytes(), tags.tobytes(), name_offs.tobytes(), np.full(na, 0o644, np.uint16).tobytes(), name_data])


def parse_version_index(vi):
    h = np.frombuffer(vi[:24], np.uint32)
    na, nu, ni = int(h[3]), int(h[4]), int(h[5])
    o = 24 + na * 16
    out = dict(hash_id=int(h[1]), target=int(h[2]))
    for name, dt, n in (("sizes", np.uint64, na), ("counts", np.uint32, na), ("starts", np.uint32, na), ("idx", np.uint32, ni),
                        ("chunk_hashes", np.uint64, nu), ("chunk_sizes", np.uint32, nu), ("chunk_tags", np.uint32, nu)):
        nbytes = n * np.dtype(dt).itemsize
        out[name] = np.frombuffer(vi[o : o + nbytes], dt).copy()
        o += nbytes
    return out


def build_store_index(hash_id, blocks, chunk_hashes, chunk_sizes):
    """blocks: [(block hash, tag, [indices into the chunk lists])]; the index lists each block's chunks in turn."""
    nb = len(blocks)
    order = [c for _, _, cs in blocks for c in cs]
    counts = np.array([len(cs) for _, _, cs in blocks], np.uint32)
    offs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32) if nb else np.zeros(0, np.uint32)
    head = np.array([STORE_INDEX_VERSION, hash_id if order else 0, nb, len(order)], np.uint32)
    return b"".join([head.tobytes(), np.array([b for b, _, _ in blocks], np.uint64).tobytes(),
                     np.asarray(chunk_hashes, np.uint64)[order].tobytes(), offs.tobytes(), counts.tobytes(),
                     np.array([t for _, t, _ in blocks], np.uint32).tobytes(), np.asarray(chunk_sizes, np.uint32)[order].tobytes()])


def parse_store_index(si):
    h = np.frombuffer(si[:16], np.uint32)
    nb, m = int(h[2]), int(h[3])
    o = 16
    out = dict(hash_id=int(h[1]))
    for name, dt, n in (("block_hashes", np.uint64, nb), ("chunk_hashes", np.uint64, m), ("block_offsets", np.uint32, nb),
                        ("block_counts", np.uint32, nb), ("block_tags", np.uint32, nb), ("chunk_sizes", np.uint32, m)):
        nbytes = n * np.dtype(dt).itemsize
        out[name] = np.frombuffer(si[o : o + nbytes], dt).copy()
        o += nbytes
    return out


def without_last_block(si):
    """The same StoreIndex without its last block (and that block's chunks)."""
    p = parse_store_index(si)
    nb = len(p["block_hashes"]) - 1
    m = int(p["block_offsets"][nb])
    head = np.array([STORE_INDEX_VERSION, p["hash_id"] if m else 0, nb, m], np.uint32)
    return b"".join([head.tobytes(), p["block_hashes"][:nb].tobytes(), p["chunk_hashes"][:m].tobytes(), p["block_offsets"][:nb].tobytes(),
                     p["block_counts"][:nb].tobytes(), p["block_tags"][:nb].tobytes(), p["chunk_sizes"][:m].tobytes()])


def block_index_bytes(block_hash, hash_id, tag, chunk_hashes, chunk_sizes):
    return b"".join([np.array([block_hash], np.uint64).tobytes(), np.array([hash_id, len(chunk_hashes), tag], np.uint32).tobytes(),
                     np.asarray(chunk_hashes, np.uint64).tobytes(), np.asarray(chunk_sizes, np.uint32).tobytes()])


def raw_image(block_hash, hash_id, chunk_hashes, chunk_sizes, content):
    """The tag-0 image: BlockIndex + the chunks' bytes."""
    return np.frombuffer(block_index_bytes(block_hash, hash_id, 0, chunk_hashes, chunk_sizes) + bytes(content), np.uint8).copy()


def numpy_layout(sizes, align):
    offs, at = [], 0
    for s in sizes:
        at = (at + align - 1) // align * align
        offs.append(at)
        at += int(s)
    return np.array(offs, np.uint64), at
