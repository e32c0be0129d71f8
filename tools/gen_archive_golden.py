#!/usr/bin/env python3
"""Generates tests/golden/archive_ref.npz from the REFERENCE (run in the build container only; needs oracle/_ref/liblongtail_ref.so).
The output is DATA: a small one-file archive as the reference lays it out, and the assets it restores to.

  archive      [index][body]: the index is the bytes of Longtail_CreateArchiveIndex (pad bytes as the reference left them, made
               deterministic here by zeroing), with the blocks in SHUFFLED order at ODD body offsets in its tables; the body holds six
               stored blocks: two raw, two whose payload the reference's LZ4 wrote, two whose payload the reference's zstd wrote
  index_bytes  the size of the index
  assets       the bytes of every asset of the VersionIndex, back to back; asset_sizes their sizes
tests/test_gpu_archive.py restores the archive and compares with the assets; it runs without the reference."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests._libs import GOLDEN, oracle, ref  # noqa: E402
from tests.archive_util import RefArchive, place, tagged_image  # noqa: E402
from tests.restore_util import BLK3, build_store_index, build_version_index, raw_image  # noqa: E402


def main():
    o, r = oracle(), ref()
    rng = np.random.default_rng(2024)
    tags = [0, r.lz4_type, r.zstd_default, 0, r.zstd_default, r.lz4_type]
    lens, blocks, at = [], [], 0
    for b, tag in enumerate(tags):
        n = [3, 7, 5, 1, 9, 4][b]
        blocks.append((0xA5C4000 + b, tag, list(range(at, at + n))))
        lens += [int(x) for x in rng.integers(300, 1800, n)]
        at += n
    # text of a 64-word vocabulary: matches at many distances and lengths, literals in between
    words = [rng.integers(0, 256, int(n)).astype(np.uint8) for n in rng.integers(2, 14, 64)]
    content = np.concatenate([words[int(w)] for w in rng.integers(0, 64, sum(lens))])[: sum(lens)].copy()
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    hashes = o.blake3_many(content, starts, lens)
    piece = lambda c: content[int(starts[c]) : int(starts[c]) + lens[c]]
    images = []
    for bh, tag, cs in blocks:
        body = np.concatenate([piece(c) for c in cs])
        h, s = hashes[cs], np.array(lens, np.uint32)[cs]
        if not tag:
            images.append(raw_image(bh, BLK3, h, s, body.tobytes()))
        else:
            payload = r.compress(0 if tag == r.lz4_type else 1, tag, body)
            assert len(payload) < len(body)
            images.append(tagged_image(bh, BLK3, tag, h, s, payload.tobytes(), len(body)))
    asset_chunks = [cs for _, _, cs in blocks] + [[cs[0] for _, _, cs in blocks], []]
    names = [f"dir/file{b}.bin" for b in range(len(blocks))] + ["first_chunks.bin", "empty.bin"]
    vi = build_version_index(BLK3, 1024, names, asset_chunks, hashes, lens, chunk_tags=[t for _, t, cs in blocks for _ in cs])
    si = build_store_index(BLK3, blocks, hashes, lens)
    order = [4, 1, 5, 0, 3, 2]  # the order the blocks lie in the body
    offsets, at = [0] * len(images), 1
    for b in order:
        offsets[b] = at
        at += len(images[b]) + (2 if (at + len(images[b])) % 2 else 1)  # every offset odd
    assert all(x % 2 for x in offsets)
    body = place(images, offsets)
    index = RefArchive(r).create(si, vi, offsets, [len(i) for i in images])
    assert isinstance(index, bytes), index
    bare = 8 + len(si) + 12 * len(images) + len(vi)
    index = index[:bare] + bytes(len(index) - bare)  # (the reference leaves the pad uninitialised)
    archive = np.concatenate([np.frombuffer(index, np.uint8), body])
    assets = [np.concatenate([piece(c) for c in cs]) if cs else np.zeros(0, np.uint8) for cs in asset_chunks]
    out = GOLDEN / "archive_ref.npz"
    np.savez_compressed(out, archive=archive, index_bytes=np.array([len(index)], np.uint64), assets=np.concatenate(assets),
                        asset_sizes=np.array([len(a) for a in assets], np.uint64))
    print(out, out.stat().st_size, "bytes; archive", len(archive), "index", len(index))
    assert out.stat().st_size <= 64 << 10


if __name__ == "__main__":
    main()
