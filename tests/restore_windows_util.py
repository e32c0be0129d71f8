"""Helpers of the window-restore tests (lthip_restore_create_windows, include/longtail_hip.h "byte windows of assets"): the hand-built
version of the clip sweep and its windows, the tree of the rank-share test, and Python models of the three host routines of
longtail_amd/csrc/restore_windows.h -- the expansion of windows into clipped occurrences, the rank's window table, the expected output."""
import numpy as np

from tests.restore_util import BLK3, build_store_index, build_version_index, parse_version_index

FILL = 0xA5

# ---- the clip sweep: 7 chunks in three blocks, every chunk in all three assets at another position ----
LENGTHS = [1, 15, 16, 17, 33, 255, 4097]
SWEEP_BLOCKS = [[0, 1, 2], [3, 4], [5, 6]]
SWEEP_ASSETS = [[0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0], [3, 0, 6, 1, 5, 2, 4, 0]]
SKIPS = lambda n: sorted({s for s in (0, 1, 2, 3, 5, 16, n - 1) if 0 <= s < n})
CLIPS = lambda n, skip: sorted({c for c in (1, 2, 15, 16, 17, n - skip) if 1 <= c <= n - skip})


def sweep_chunks(seed=21):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n).astype(np.uint8) for n in LENGTHS]


def sweep_version(hashes, block_hashes=(11, 12, 13)):
    """-> (vi, si) of the sweep's three assets and three raw blocks, for the given chunk hashes."""
    vi = build_version_index(BLK3, 32768, [f"s{a}" for a in range(len(SWEEP_ASSETS))], SWEEP_ASSETS, hashes, LENGTHS)
    si = build_store_index(BLK3, [(int(h), 0, cs) for h, cs in zip(block_hashes, SWEEP_BLOCKS)], hashes, LENGTHS)
    return vi, si


def sweep_files(chunks):
    return [np.concatenate([chunks[c] for c in cs]) for cs in SWEEP_ASSETS]


def place(spans):
    """(asset, offset, length) -> (asset, offset, length, dst): window i lands at destination residue i mod 16, behind the one before it
    with a gap that must keep its fill.  -> (rows, out_bytes)"""
    rows, at = [], 0
    for i, (a, off, n) in enumerate(spans):
        at = (at + 15) // 16 * 16 + 16 + i % 16
        rows.append((a, off, n, at))
        at += n
    return rows, at + 32


def sweep_windows():
    """Every chunk with every (skip, clip) of the lists, taken at every position the chunk has in the three assets in turn; then windows
    over two and three chunks that start and end on chunk boundaries, and ones that start or end one byte off a boundary."""
    spans, turn = [], 0
    where = {}  # chunk -> [(asset, where the chunk starts in it)]
    for a, cs in enumerate(SWEEP_ASSETS):
        at = 0
        for c in cs:
            where.setdefault(c, []).append((a, at))
            at += LENGTHS[c]
    for c, n in enumerate(LENGTHS):
        assert len({a for a, _ in where[c]}) >= 2
        for skip in SKIPS(n):
            for clip in CLIPS(n, skip):
                a, begin = where[c][turn % len(where[c])]
                turn += 1
                spans.append((a, begin + skip, clip))
    for a, cs in enumerate(SWEEP_ASSETS):
        bounds = np.concatenate([[0], np.cumsum([LENGTHS[c] for c in cs])]).tolist()
        for k in range(len(cs)):
            for span in (2, 3):
                if k + span > len(cs):
                    continue
                lo, hi = bounds[k], bounds[k + span]
                spans.append((a, lo, hi - lo))  # boundary to boundary
                spans.append((a, lo + 1, hi - lo - 1))  # a byte into the first chunk
                spans.append((a, lo, hi - lo - 1))  # a byte short of the last chunk's end
                if k:
                    spans.append((a, lo - 1, hi - lo + 2 if hi < bounds[-1] else hi - lo + 1))  # a byte of the neighbours
    return place(spans)


# ---- the models ----


def model_occurrences(vi, windows):
    """restore_windows::expand -> [(chunk hash, full length, skip, clip, destination)] in window and chunk order, and the number of
    distinct assets named.  A window plans the chunks from the one that holds its first byte to the one that holds its last."""
    p = parse_version_index(vi)
    occ, named = [], set()
    for a, off, n, dst in windows:
        a, off, n, dst = int(a), int(off), int(n), int(dst)
        named.add(a)
        if not n:
            continue
        idx = p["idx"][int(p["starts"][a]) : int(p["starts"][a]) + int(p["counts"][a])]
        sizes = p["chunk_sizes"][idx].astype(np.int64)
        pre = np.concatenate([[0], np.cumsum(sizes)])
        whole = n == int(p["sizes"][a])
        first = 0 if whole else int(np.searchsorted(pre, off, side="right")) - 1
        last = len(idx) - 1 if whole else int(np.searchsorted(pre, off + n - 1, side="right")) - 1
        for k in range(first, last + 1):
            lo, hi = max(int(pre[k]), off), min(int(pre[k + 1]), off + n)
            occ.append((int(p["chunk_hashes"][idx[k]]), int(sizes[k]), lo - int(pre[k]), hi - lo, dst + lo - off))
    return occ, len(named)


def expected_windows_output(files, windows, out_bytes):
    out = np.full(out_bytes, FILL, np.uint8)
    for a, off, n, dst in windows:
        out[int(dst) : int(dst) + int(n)] = files[int(a)][int(off) : int(off) + int(n)]
    return out


def model_rank_windows(job_asset, job_offset, job_size, job_rank, rank, align):
    """restore_windows::rank_windows -> (rows of (asset, offset, length, dst), out_bytes)."""
    rows, end = [], 0
    for a, off, n, r in zip(job_asset.tolist(), job_offset.tolist(), job_size.tolist(), job_rank.tolist()):
        if r != rank or not n:
            continue
        if rows and rows[-1][0] == a and rows[-1][1] + rows[-1][2] == off:
            rows[-1][2] += n
        else:
            rows.append([a, off, n, (end + align - 1) // align * align])
        end = rows[-1][3] + rows[-1][2]
    return [tuple(r) for r in rows], end


# ---- the tree of the rank-share test: target 1, so parts are 1 KiB and the jobs are many ----
SHARE_SIZES = [0, 1, 1023, 1024, 1025, 5000, 0]
SHARE_NAMES = ["empty", "one", "k-1", "k", "k+1", "five", "dir/"]
SHARE_CHUNK = 700  # every file is cut into chunks of 700 bytes (the last one shorter), no chunk shared


def share_tree(seed=33):
    """-> (files, chunk contents, per asset its chunk indices, chunk lengths, blocks: three lists of chunk indices)."""
    rng = np.random.default_rng(seed)
    files = [rng.integers(0, 256, n).astype(np.uint8) for n in SHARE_SIZES]
    chunks, asset_chunks = [], []
    for f in files:
        mine = []
        for o in range(0, len(f), SHARE_CHUNK):
            mine.append(len(chunks))
            chunks.append(f[o : o + SHARE_CHUNK])
        asset_chunks.append(mine)
    lens = [len(c) for c in chunks]
    order = list(range(len(chunks)))
    blocks = [order[0::3], order[1::3], order[2::3]]
    return files, chunks, asset_chunks, lens, blocks
