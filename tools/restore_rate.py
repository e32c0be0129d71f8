#!/usr/bin/env python3
"""Rate of the restore session (lthip_restore_*): a `mixed` tree of 1 MiB files is written by the stream ingest session (one slice, the
images stay in HBM) and restored from those images into a device buffer -- raw (tag 0), LZ4 and zstd stores, each with verify off and
on.  Timed: every lthip_restore_blocks call and lthip_restore_finish (the session's one synchronisation); lthip_restore_create -- the
plan -- is timed by itself.  Beside each figure: the time of the BARE lthip_*_decompress_blocks call over the same blocks into the same
kind of scratch, in the same process -- what the library could already do; the session's overhead (image check, verify, scatter) is the
difference.  The output is compared with the tree once per store.  Recorded into profiles/restore_rate.json: GB/s of output of every
repeat.  There is no threshold.

    python tools/restore_rate.py [--gib 4] [--repeats 3] [--out profiles/restore_rate.json]
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
TAGS = {"none": 0, "lz4": 0x6C7A3432, "zstd": 0x7A746432}


def store_blocks(si):
    h = np.frombuffer(si[:16], np.uint32)
    nb, m = int(h[2]), int(h[3])
    o = 16
    hashes = np.frombuffer(si[o : o + nb * 8], np.uint64).copy()
    o += nb * 8 + m * 8
    first = np.frombuffer(si[o : o + nb * 4], np.uint32).astype(np.int64)
    count = np.frombuffer(si[o + nb * 4 : o + nb * 8], np.uint32).astype(np.int64)
    o += nb * 12
    sizes = np.frombuffer(si[o : o + m * 4], np.uint32).astype(np.int64)
    cs = np.concatenate([[0], np.cumsum(sizes)])
    return hashes, count, cs[first + count] - cs[first]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--target-chunk-size", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=8 << 20)
    ap.add_argument("--max-chunks-per-block", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "restore_rate.json"))
    args = ap.parse_args()

    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Context, Ingest, IngestStream, Restore, chunker_params, load

    lib = load()
    dev = torch.device("cuda", 0)
    ctx = Context(0, lib=lib)
    nfiles = int(args.gib * (1 << 30)) // FILE
    n = nfiles * FILE
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off, p_size = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE), np.full(nfiles, FILE, np.uint64)
    u8 = dict(dtype=torch.uint8, device=dev)
    data = torch.empty(n + 256, **u8)
    ctx.synth_fill(data, p_off, p_size, asset_seeds(0x10C0FFEE, 0, nfiles), KINDS["mixed"])
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)
    total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, data)
    tree = make_tree("files", n, FILE)
    whole, _keep = Ingest.tree(tree["sizes"], tree["path_offsets"], tree["perms"], tree["path_data"], np.arange(nfiles, dtype=np.uint32),
                               np.zeros(nfiles + 1, np.uint64))
    vi_cap = int(lib.dll.lthip_version_index_size(nfiles, total, total, len(tree["path_data"]))) + 64
    h_vi, h_si = torch.empty(vi_cap, dtype=torch.uint8).pin_memory(), torch.empty(16 + 32 * total + 64, dtype=torch.uint8).pin_memory()
    out = torch.empty(n, **u8)
    report = {"workload": f"{args.gib:g} GiB `mixed` tree ({nfiles} files of 1 MiB), written by lthip_ingest_stream in one slice, restored from its "
                          "images in HBM into a device buffer: all lthip_restore_blocks calls + lthip_restore_finish",
              "unit": "GB/s of output", "repeats": args.repeats, "stores": {}}
    for codec, tag in TAGS.items():
        st = IngestStream(ctx, whole, args.target_chunk_size, args.block_size, args.max_chunks_per_block, codec, compression_type=tag or None)
        arena, tail = torch.empty(st.arena_bound(n, total), **u8), torch.empty(st.arena_bound(0, 0), **u8)
        st.slice(0, nfiles, data, d_off, d_len, d_hash, d_first, total, arena)
        _, offs0, sizes0 = st.images()
        offs0, sizes0 = offs0.copy(), sizes0.copy()
        res = st.finish(tail, h_vi, h_si)
        _, offs1, sizes1 = st.images()
        offs1, sizes1 = offs1.copy(), sizes1.copy()
        vi, si = bytes(h_vi.numpy()[: res.version_index_size]), bytes(h_si.numpy()[: res.store_index_size])
        st.close()
        hashes, counts, raws = store_blocks(si)
        calls = [(arena, hashes[: len(offs0)], offs0, sizes0), (tail, hashes[len(offs0) :], offs1, sizes1)]
        assert len(hashes) == len(offs0) + len(offs1) == res.blocks
        offsets, out_bytes = Restore.layout(vi, 1, lib)
        assert out_bytes == n
        entry = {"blocks": int(res.blocks), "raw_bytes_of_the_blocks": int(raws.sum()), "stored_bytes": int(sizes0.astype(np.int64).sum() + sizes1.astype(np.int64).sum())}
        scratch = None
        for verify in (False, True):
            plans, rates = [], []
            for rep in range(args.repeats + 1):  # (the first is the warm-up: workspaces of the context)
                out.fill_(0xA5)
                ctx.sync()
                t0 = time.perf_counter()
                rs = Restore(ctx, vi, si, offsets, n, verify=verify)
                t1 = time.perf_counter()
                if scratch is None:
                    bound = max(rs.scratch_bound(h) for _, h, _, _ in calls)
                    scratch = torch.empty(max(bound, 64), **u8)
                    ctx.sync()
                    t1 = time.perf_counter()
                for images, h, o, z in calls:
                    if len(h):
                        rs.blocks(h, images, o, z, scratch, out)
                code, result = rs.finish()
                t2 = time.perf_counter()
                assert code == 0 and result.bytes_written == n, (code, result.bytes_written)
                if rep == 0:
                    assert torch.equal(out, data[:n]), "the restored bytes differ from the tree"
                else:
                    plans.append(round((t1 - t0) * 1e3, 2))
                    rates.append(round(n / (t2 - t1) / 1e9, 2))
                rs.close()
            entry["verify" if verify else "no_verify"] = {"GBps": rates, "GBps_median": float(np.median(rates)), "create_ms": plans}
        if codec != "none":  # the bare decoder call over the same blocks, into the same scratch
            decode = ctx.lz4_decompress_blocks if codec == "lz4" else ctx.zstd_decompress_blocks
            hdr, k, ms = 28 + 12 * counts, 0, []
            for rep in range(args.repeats + 1):
                ctx.sync()
                t0 = time.perf_counter()
                k = 0
                for images, h, o, z in calls:
                    if len(h):
                        r = raws[k : k + len(h)]
                        slots = np.concatenate([[0], np.cumsum((r + 63) // 64 * 64)[:-1]])
                        decode(images, o.astype(np.int64) + hdr[k : k + len(h)], z.astype(np.int64) - hdr[k : k + len(h)], scratch, slots, r)
                        k += len(h)
                ctx.sync()
                if rep:
                    ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            entry["bare_decoder_ms"] = ms  # (it decodes the store's unique bytes once; the session also writes every duplicate)
            entry["bare_decoder_GBps_of_decoded_bytes_median"] = round(int(raws.sum()) / (float(np.median(ms)) * 1e-3) / 1e9, 2)
        report["stores"][codec] = entry
        print(codec, json.dumps(entry), flush=True)
        del arena, tail, scratch
    plan.close()
    ctx.close()
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
