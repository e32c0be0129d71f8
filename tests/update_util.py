"""Helpers of the update tests (a base for the restore session, lthip_version_diff): a serialized VersionIndex whose path hashes, content
hashes and permissions the caller chooses (tests/restore_util.py fixes all three), layout src/longtail.c:2551-2584, and a reader for the
per-asset fields."""
import numpy as np

from tests.restore_util import VERSION_INDEX_VERSION


def build_version_index(hash_id, target, names, asset_chunks, chunk_hashes, chunk_sizes, path_hashes=None, content_hashes=None, permissions=None,
                        chunk_tags=None):
    """names[a]: the asset's path (a directory ends with '/'); asset_chunks[a]: indices into the unique chunk lists.  Defaults: path hash
    a + 1, content hash a + 101, permissions 0o644 (what tests/restore_util.py writes)."""
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
    ph = np.arange(1, na + 1, dtype=np.uint64) if path_hashes is None else np.asarray(path_hashes, np.uint64)
    ch = np.arange(101, na + 101, dtype=np.uint64) if content_hashes is None else np.asarray(content_hashes, np.uint64)
    pm = np.full(na, 0o644, np.uint16) if permissions is None else np.asarray(permissions, np.uint16)
    assert len(ph) == len(ch) == len(pm) == na
    return b"".join([head.tobytes(), ph.tobytes(), ch.tobytes(), sizes.tobytes(), counts.tobytes(), starts.tobytes(), idx.tobytes(),
                     np.asarray(chunk_hashes, np.uint64).tobytes(), chunk_sizes.tobytes(), tags.tobytes(), name_offs.tobytes(), pm.tobytes(),
                     name_data])


def asset_fields(vi):
    """-> dict(path_hashes, content_hashes, permissions, names) of a serialized VersionIndex."""
    h = np.frombuffer(vi[:24], np.uint32)
    na, nu, ni = int(h[3]), int(h[4]), int(h[5])
    ph = np.frombuffer(vi[24 : 24 + na * 8], np.uint64).copy()
    ch = np.frombuffer(vi[24 + na * 8 : 24 + na * 16], np.uint64).copy()
    o = 24 + na * 32 + ni * 4 + nu * 16
    name_offs = np.frombuffer(vi[o : o + na * 4], np.uint32)
    pm = np.frombuffer(vi[o + na * 4 : o + na * 6], np.uint16).copy()
    name_data = vi[o + na * 6 :]
    names = [name_data[int(s) : name_data.index(b"\0", int(s))].decode() for s in name_offs]
    return dict(path_hashes=ph, content_hashes=ch, permissions=pm, names=names)
