"""Helpers of the repack tests: a hand-built store in the manner of tests/archive_util.hand_store whose blocks witness every rule of the
repack session's definitions (include/longtail_hip.h, "the repack session"), and a Python model of those definitions.

The store, in StoreIndex order (chunks of 1-40 bytes at odd positions):
  0..7    blocks of 1, 64, 65 and 130 chunks, each once raw and once LZ4-tagged (one run of literals)
  8, 9    two zstd-tagged blocks ('ztd1', 'ztd2'), compressed by lthip_zstd_compress_blocks in the fixture
  10      'btl1': a tag no codec of the library takes (its payload is never decoded)
  11      raw, 6 chunks of its own + chunk A of block 2 (64 raw): a chunk in a kept block and in a victim
  12, 13  LZ4 and raw, 5 chunks of their own each + the shared chunk S: a chunk in two victims
  14      raw, the same chunks as block 2 under another block hash: passes any threshold block 2 passes, and is redundant
  15      raw, 4 chunks no live set names: a block with no live chunk
"""
import numpy as np

from tests.archive_util import LZ4, lz4_literals, tagged_image
from tests.restore_util import BLK3, build_store_index, parse_store_index, raw_image

ZTD1, ZTD2, BTL1 = 0x7A746431, 0x7A746432, 0x62746C31
COUNTS = (1, 64, 65, 130)


def codec_of_tag(tag):
    return 0 if tag == 0 else 1 if tag == LZ4 else 2 if (tag >> 8) == 0x7A7464 and 0x31 <= (tag & 0xFF) <= 0x35 else -1


def hand_store(oracle, ctx, seed=11):
    """-> dict(si, blocks [(hash, tag, [chunk])], images, hashes, lens, chunks (bytes per chunk), never_live (chunk indices),
    unknown_block, shared (A, S))."""
    import torch

    rng = np.random.default_rng(seed)
    blocks, at = [], 0

    def fresh(n):
        nonlocal at
        cs = list(range(at, at + n))
        at += n
        return cs

    for k, n in enumerate(COUNTS):
        for tag in (0, LZ4):
            blocks.append((0xB10C0000 + 16 * k + (1 if tag else 0), tag, fresh(n)))
    blocks.append((0xB10C0100, ZTD1, fresh(21)))
    blocks.append((0xB10C0101, ZTD2, fresh(33)))
    blocks.append((0xB10C0200, BTL1, fresh(3)))
    a = blocks[2][2][7]
    blocks.append((0xB10C0300, 0, fresh(3) + [a] + fresh(3)))
    s = at
    at += 1
    blocks.append((0xB10C0301, LZ4, fresh(2) + [s] + fresh(3)))
    blocks.append((0xB10C0302, 0, [s] + fresh(5)))
    blocks.append((0xB10C0303, 0, list(blocks[2][2])))
    never = fresh(4)
    blocks.append((0xB10C0304, 0, never))
    lens = [int(x) for x in rng.integers(1, 41, at)]
    content = rng.integers(0, 256, sum(lens)).astype(np.uint8)
    content[: sum(lens) // 2] &= 0x0F  # (half of it compresses)
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    short = [c for c in range(at) if lens[c] <= 3]  # (so few bytes repeat by chance: their first byte counts up)
    assert len(short) < 256
    for k, c in enumerate(short):
        content[int(starts[c])] = k
    hashes = oracle.blake3_many(content, starts, lens)
    assert len(set(int(h) for h in hashes)) == len(hashes)
    piece = lambda c: content[int(starts[c]) : int(starts[c]) + lens[c]]
    images = []
    for bh, tag, cs in blocks:
        body = np.concatenate([piece(c) for c in cs])
        h, z = hashes[cs], np.array(lens, np.uint32)[cs]
        if tag == 0:
            images.append(raw_image(bh, BLK3, h, z, body.tobytes()))
        elif tag == LZ4:
            images.append(tagged_image(bh, BLK3, tag, h, z, lz4_literals(body.tobytes()), len(body)))
        elif codec_of_tag(tag) == 2 and ctx is None:  # (no device: the indexes and the model alone are wanted)
            images.append(None)
        elif codec_of_tag(tag) == 2:
            cap = len(body) + (len(body) >> 8) + 128
            dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            n = int(ctx.zstd_compress_blocks(torch.from_numpy(body).cuda(), [0], [len(body)], dst, [0], [cap]).cpu().numpy().view(np.uint32)[0])
            assert 0 < n <= cap
            images.append(tagged_image(bh, BLK3, tag, h, z, dst.cpu().numpy()[:n].tobytes(), len(body)))
        else:
            images.append(tagged_image(bh, BLK3, tag, h, z, bytes(len(body)), len(body)))
    si = build_store_index(BLK3, blocks, hashes, lens)
    return dict(si=si, blocks=blocks, images=images, hashes=hashes, lens=lens, chunks=[piece(c) for c in range(at)], never_live=never,
                unknown_block=10, shared=(a, s), block_hashes=parse_store_index(si)["block_hashes"])


def live_sets(st):
    """The live lists of the tests (chunk indices, with duplicates): all but the never-live chunks and those of the block with the
    unknown tag (which must not become a source: the create refusals test that block on its own); every second of those; one; none."""
    never = set(st["never_live"]) | set(st["blocks"][st["unknown_block"]][2])
    every = [c for _, _, cs in st["blocks"] for c in cs if c not in never]  # (block order: the shared chunks come twice)
    return {"all": every, "every second chunk": every[::2], "one chunk": [st["blocks"][3][2][5]], "none": []}


def model(st, live_chunks, percent):
    """The definitions in Python -> dict(kept (block indices, in the walk's order), moved (chunk indices, live order), sources, dropped,
    moved_tags, moved_lens)."""
    blocks, lens = st["blocks"], st["lens"]
    live = list(dict.fromkeys(live_chunks))
    wanted = set(live)
    pct, cand = {}, []
    for b, (_, _, cs) in enumerate(blocks):
        use, size = sum(lens[c] for c in cs if c in wanted), sum(lens[c] for c in cs)
        if use == 0:
            continue
        pct[b] = use * 100 // size
        if percent > 0 and pct[b] < percent:
            continue
        cand.append(b)
    cand.sort(key=lambda b: -pct[b])  # (stable: equal usages in store order)
    kept, claimed = [], set()
    for b in cand:
        mine = [c for c in blocks[b][2] if c in wanted and c not in claimed]
        if mine:
            kept.append(b)
            claimed.update(c for c in blocks[b][2] if c in wanted)
    held = {c for b in kept for c in blocks[b][2]}
    moved = [c for c in live if c not in held]
    first_block = {}
    for b, (_, _, cs) in enumerate(blocks):
        for c in cs:
            first_block.setdefault(c, b)
    sources = sorted({first_block[c] for c in moved})
    dropped = [b for b in range(len(blocks)) if b not in kept]
    return dict(kept=kept, moved=moved, sources=sources, dropped=dropped, moved_tags=[blocks[first_block[c]][1] for c in moved],
                moved_lens=[lens[c] for c in moved], live=live)


def source_block_of(st):
    """chunk -> its source block: the first block in StoreIndex order that holds it."""
    first = {}
    for b, (_, _, cs) in enumerate(st["blocks"]):
        for c in cs:
            first.setdefault(c, b)
    return first


def own_tags(kept_index: bytes, store_index: bytes) -> bytes:
    """kept_index with every block's tag word set to what store_index records for the block of that hash."""
    k, s = parse_store_index(kept_index), parse_store_index(store_index)
    tag_of = {}
    for h, t in zip(s["block_hashes"], s["block_tags"]):
        tag_of.setdefault(int(h), int(t))
    nb, m = len(k["block_hashes"]), len(k["chunk_hashes"])
    at = 16 + 8 * nb + 8 * m + 8 * nb
    tags = np.array([tag_of[int(h)] for h in k["block_hashes"]], np.uint32).tobytes()
    return kept_index[:at] + tags + kept_index[at + 4 * nb :]


def decoded_new_blocks(st, new_index: bytes):
    """The expected content of every new block: [(tag, [chunk hashes], [sizes], content bytes)] in the new index's order."""
    p = parse_store_index(new_index)
    by_hash = {int(h): c for c, h in enumerate(st["hashes"])}
    out = []
    for b in range(len(p["block_hashes"])):
        o, n = int(p["block_offsets"][b]), int(p["block_counts"][b])
        hs, zs = p["chunk_hashes"][o : o + n], p["chunk_sizes"][o : o + n]
        body = b"".join(st["chunks"][by_hash[int(h)]].tobytes() for h in hs)
        out.append((int(p["block_tags"][b]), hs, zs, body))
    return out
