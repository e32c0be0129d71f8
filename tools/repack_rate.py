#!/usr/bin/env python3
"""Rate of the repack session (lthip_repack_*) beside the path an embedder has without it.

A `mixed` tree of 1 MiB files is version 1; versions 2, 3 and 4 each replace another tenth of the files of the version before.  Every
version is written by the stream ingest session against a store that holds the versions before it (one slice each, the images stay in
HBM), so the store is the four StoreIndexes merged.  The last --keep versions (default 2) are kept: the oldest version's blocks are
partly dead.  Then, in one process and alternated repeat by repeat, for min_block_usage_percent 50 and 90:

  repack    lthip_repack_create (timed by itself), then every lthip_repack_blocks call over the source blocks where they lie,
            lthip_repack_write and lthip_repack_finish
  baseline  what an embedder does today: every kept version restored from the store into a device buffer (lthip_restore_*, verify off),
            chunked and hashed again (lthip_chunk_hash) and stream-ingested with set_store into a store that starts empty

Buffers are allocated outside the timing on both sides.  Once per percent the newest version is restored, with verify, from the index
and the images the repack left and compared with its bytes.  Recorded into profiles/repack_rate.json: milliseconds of create and of
blocks + write + finish, moved bytes, blocks kept / dropped / new, the baseline's milliseconds and the ratio.  There is no threshold.

    python tools/repack_rate.py [--gib 4] [--repeats 3] [--codec lz4] [--keep 2] [--out profiles/repack_rate.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FILE = 1 << 20
VERSIONS = 4


def block_hashes(si):
    nb = int(np.frombuffer(si[8:12], np.uint32)[0])
    return np.frombuffer(si[16 : 16 + nb * 8], np.uint64).copy()


def block_raw_sizes(si):
    """-> (block hashes as ints, the sums of their chunk sizes)"""
    h = np.frombuffer(si[:16], np.uint32)
    nb, m = int(h[2]), int(h[3])
    o = 16 + nb * 8 + m * 8
    first = np.frombuffer(si[o : o + nb * 4], np.uint32).astype(np.int64)
    count = np.frombuffer(si[o + nb * 4 : o + nb * 8], np.uint32).astype(np.int64)
    sizes = np.frombuffer(si[o + nb * 12 : o + nb * 12 + m * 4], np.uint32).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(sizes)])
    return [int(x) for x in block_hashes(si)], [int(x) for x in cs[first + count] - cs[first]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--codec", default="lz4", choices=["none", "lz4", "zstd"])
    ap.add_argument("--keep", type=int, default=2, help="how many of the newest versions stay")
    ap.add_argument("--share", type=float, default=0.1, help="the share of the files every version replaces")
    ap.add_argument("--target-chunk-size", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=8 << 20)
    ap.add_argument("--max-chunks-per-block", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "repack_rate.json"))
    args = ap.parse_args()

    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Context, Ingest, IngestStream, Repack, Restore, Store, chunker_params, load, store_index_merge, version_chunk_hashes

    lib = load()
    ctx = Context(0, lib=lib)
    u8 = dict(dtype=torch.uint8, device=torch.device("cuda", 0))
    nfiles = max(VERSIONS * 10, int(args.gib * (1 << 30)) // FILE)
    n = nfiles * FILE
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off, p_size = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE), np.full(nfiles, FILE, np.uint64)
    tree = make_tree("files", n, FILE)
    whole, _keep = Ingest.tree(tree["sizes"], tree["path_offsets"], tree["perms"], tree["path_data"], np.arange(nfiles, dtype=np.uint32),
                               np.zeros(nfiles + 1, np.uint64))
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)
    step = max(1, round(1 / args.share))
    # ---- the versions' bytes ----
    data = [torch.empty(n + 256, **u8)]
    ctx.synth_fill(data[0], p_off, p_size, asset_seeds(0x10C0FFEE, 0, nfiles), KINDS["mixed"])
    for v in range(1, VERSIONS):
        replaced = np.arange(v - 1, nfiles, step)
        data.append(data[-1].clone())
        ctx.synth_fill(data[-1], p_off[replaced], p_size[replaced], asset_seeds(0xB0B0CAFE + v, 0, len(replaced)), KINDS["mixed"])
    ctx.sync()

    def ingest(src, store, arena=None, tail=None, buffers=None, chunks_bound=0):
        """-> (vi, si, calls [(images, hashes, offsets, sizes)]) of the tree in `src`, one slice, against `store` (or none); chunks_bound:
        the arena and the index buffers are made for a version of that many chunks"""
        total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, src)
        st = IngestStream(ctx, whole, args.target_chunk_size, args.block_size, args.max_chunks_per_block, args.codec)
        if store is not None:
            st.set_store(store)
        if buffers is None:
            room = max(total, chunks_bound)
            vi_cap = int(lib.dll.lthip_version_index_size(nfiles, room, room, len(tree["path_data"]))) + 64
            buffers = (torch.empty(vi_cap, dtype=torch.uint8).pin_memory(), torch.empty(16 + 32 * room + 64, dtype=torch.uint8).pin_memory())
        arena = torch.empty(st.arena_bound(n, max(total, chunks_bound)), **u8) if arena is None else arena
        tail = torch.empty(st.arena_bound(0, 0), **u8) if tail is None else tail
        st.slice(0, nfiles, src, d_off, d_len, d_hash, d_first, total, arena)
        _, offs0, sizes0 = st.images()
        res = st.finish(tail, *buffers)
        _, offs1, sizes1 = st.images()
        vi, si = bytes(buffers[0].numpy()[: res.version_index_size]), bytes(buffers[1].numpy()[: res.store_index_size])
        st.close()
        hashes = block_hashes(si)
        return vi, si, [(arena, hashes[: len(offs0)], offs0.copy(), sizes0.copy()), (tail, hashes[len(offs0) :], offs1.copy(), sizes1.copy())], (arena, tail, buffers)

    # ---- the store: every version against the ones before it ----
    known = Store(ctx, 0)
    vis, si_all, calls_all = [], None, []
    for v in range(VERSIONS):
        vi, si, calls, (arena, tail, _) = ingest(data[v], known if v else None)
        known.add_index(si)
        vis.append(vi)
        si_all = si if si_all is None else store_index_merge(si_all, si)
        used = max(64, int((calls[0][2].astype(np.int64) + calls[0][3].astype(np.int64)).max()) if len(calls[0][2]) else 0)
        calls_all += [(arena[:used].clone(), *calls[0][1:]), calls[1]]
        del arena
    known.close()
    kept_versions = list(range(VERSIONS - args.keep, VERSIONS))
    live = torch.from_numpy(np.concatenate([version_chunk_hashes(vis[v]) for v in kept_versions]).view(np.int64)).cuda()
    offsets, out_bytes = Restore.layout(vis[-1], 1, lib)
    assert out_bytes == n
    out = torch.empty(n + 256, **u8)
    spare = ingest(data[-1], None, chunks_bound=int(plan.capacity))[3]  # the baseline's arena, tail and index buffers, allocated once

    def picked(calls, wanted):
        """per call (images, hashes, offsets, sizes) of its blocks whose hash is among `wanted`: host tables, made outside every timing"""
        wanted = set(int(h) for h in wanted)
        table = []
        for images, h, o, z in calls:
            pick = [i for i, x in enumerate(h) if int(x) in wanted]
            table.append((images, h[pick], o[pick], z[pick]))
        return table

    def restore(vi, si, calls, verify, scratch, needed_calls=None):
        """needed_calls: `calls` cut down to the session's needed blocks already (the baseline's are made once, outside its timing)"""
        rs = Restore(ctx, vi, si, offsets, n, verify=verify)
        for images, h, o, z in needed_calls if needed_calls is not None else picked(calls, rs.needed_blocks()):
            if len(h):
                rs.blocks(h, images, o, z, scratch, out)
        code, result = rs.finish()
        assert code == 0 and result.bytes_written == n, (code, result.bytes_written)
        rs.close()

    # a scratch that decodes every block of any one call: 64-byte slots of the blocks' raw sizes (none for a store of raw blocks)
    raw_of = dict(zip(*block_raw_sizes(si_all)))
    per_call = [sum((raw_of[int(x)] + 63) // 64 * 64 for x in h) for _, h, _, _ in calls_all]
    scratch = torch.empty(max(64, max(per_call) if args.codec != "none" else 0), **u8)

    needed_of = {}
    for v in kept_versions:  # which blocks a restore of every kept version needs, and where they lie: host tables the embedder has
        probe = Restore(ctx, vis[v], si_all, offsets, n, verify=False)
        needed_of[v] = picked(calls_all, probe.needed_blocks())
        probe.close()

    def baseline():
        fresh = Store(ctx, 0)
        ctx.sync()
        t0 = time.perf_counter()
        for k, v in enumerate(kept_versions):
            restore(vis[v], si_all, calls_all, False, scratch, needed_of[v])
            _, si, _, _ = ingest(out, fresh if k else None, *spare)
            fresh.add_index(si)
        ctx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        fresh.close()
        return ms

    def repack(percent, check):
        ctx.sync()
        t0 = time.perf_counter()
        rp = Repack(ctx, si_all, live, percent, args.block_size, args.max_chunks_per_block, verify=False)
        t1 = time.perf_counter()
        info = rp.info()
        work = torch.empty(max(64, int(info.work_bytes)), **u8)
        source_calls = picked(calls_all, rp.source_blocks())
        ctx.sync()
        t2 = time.perf_counter()
        for images, h, o, z in source_calls:
            if len(h):
                rp.blocks(h, images, o, z, scratch, work)
        rp.write(work)
        code, new_index, res = rp.finish()
        t3 = time.perf_counter()
        assert code == 0, code
        if check:  # the newest version from what the repack left: the kept blocks' images where they were, the new ones in `work`
            dropped = set(int(h) for h in rp.dropped_blocks())
            left = picked(calls_all, [x for _, h, _, _ in calls_all for x in h if int(x) not in dropped])
            o_new, z_new = rp.images()
            left.append((work, block_hashes(new_index), o_new, z_new))
            out.fill_(0xA5)
            restore(vis[-1], rp.store_index(), left, True, scratch)
            assert torch.equal(out[:n], data[-1][:n]), "the newest version differs after the repack"
        entry = dict(create_ms=(t1 - t0) * 1e3, run_ms=(t3 - t2) * 1e3, moved_bytes=int(info.moved_bytes), moved_chunks=int(info.moved_chunks),
                     blocks_total=int(info.blocks_total), blocks_kept=int(info.blocks_kept), blocks_dropped=int(info.blocks_dropped),
                     blocks_source=int(info.blocks_source), new_blocks=int(info.new_blocks), work_bytes=int(info.work_bytes),
                     compressed_bytes_written=int(res.compressed_bytes_written))
        rp.close()
        return entry

    report = {"workload": f"{args.gib:g} GiB `mixed` tree ({nfiles} files of 1 MiB) in {VERSIONS} versions, each replacing every {step}th file of the "
                          f"one before; blocks written with codec {args.codec}; the newest {args.keep} versions are kept",
              "unit": "milliseconds; the ratio is baseline_ms / (create_ms + run_ms) of the medians, null where nothing moves; the sessions "
                      "of both sides are created inside their timings, the host tables of which blocks to deliver outside", "repeats": args.repeats, "percents": {}}
    for percent in (50, 90):
        create, run, base, last = [], [], [], None
        for rep in range(args.repeats + 1):  # (the first is the warm-up: workspaces of the context; it also checks the result)
            last = repack(percent, rep == 0)
            b = baseline()
            if rep:
                create.append(round(last["create_ms"], 2))
                run.append(round(last["run_ms"], 2))
                base.append(round(b, 2))
        entry = {k: v for k, v in last.items() if k not in ("create_ms", "run_ms")}
        entry.update(create_ms=create, blocks_write_finish_ms=run, baseline_restore_then_ingest_ms=base)
        # (a repack that moves nothing is its plan alone: a ratio to the baseline would say nothing)
        entry["baseline_over_repack"] = round(float(np.median(base)) / (float(np.median(create)) + float(np.median(run))), 2) if entry["moved_bytes"] else None
        report["percents"][str(percent)] = entry
        print(percent, json.dumps(entry), flush=True)
    plan.close()
    ctx.close()
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
