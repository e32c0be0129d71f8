#!/usr/bin/env python3
"""Rates of the one-file archive (lthip_archive_*, lthip_restore_archive_blocks): a `mixed` tree of 1 MiB files is written by the stream
ingest session (one slice, the images stay in HBM), packed into an archive body by an ArchiveWriter and restored from that body -- raw
(tag 0), LZ4 and zstd stores.  Two things are measured, each beside its yardstick in the same process:

  pack      the two lthip_archive_writer_append calls (k_archive_pack) between two synchronisations, beside a device-to-device torch copy
            of as many bytes -- that copy, not the code under test, is what the kernel is measured against
  restore   lthip_restore_archive_blocks over the whole body (one window) + lthip_restore_finish, beside the same restore from the 8-byte
            aligned images the session left (lthip_restore_blocks + finish), alternated repeat by repeat, verify off and on.  The
            unaligned check touches headers only: the expectation is a ratio inside the spread of the repeats

The restored bytes are compared with the tree once per store.  Recorded into profiles/archive_rate.json.  There is no threshold.

    python tools/archive_rate.py [--gib 4] [--repeats 3] [--out profiles/archive_rate.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

FILE = 1 << 20
TAGS = {"none": 0, "lz4": 0x6C7A3432, "zstd": 0x7A746432}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--target-chunk-size", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=8 << 20)
    ap.add_argument("--max-chunks-per-block", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "archive_rate.json"))
    args = ap.parse_args()

    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Archive, ArchiveWriter, Context, Ingest, IngestStream, Restore, chunker_params, load
    from restore_rate import store_blocks

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
    report = {"workload": f"{args.gib:g} GiB `mixed` tree ({nfiles} files of 1 MiB), written by lthip_ingest_stream in one slice; its images packed "
                          "into an archive body in HBM by lthip_archive_writer_append and restored from that body in one window",
              "unit": "milliseconds; GB/s of the body (pack) and of the output (restore)", "repeats": args.repeats, "stores": {}}
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
        hashes = store_blocks(si)[0]
        calls = [(arena, hashes[: len(offs0)], offs0, sizes0), (tail, hashes[len(offs0) :], offs1, sizes1)]
        n0, n1 = int(sizes0.astype(np.int64).sum()), int(sizes1.astype(np.int64).sum())
        body, twin = torch.empty(n0 + n1, **u8), torch.empty(n0 + n1, **u8)
        # ---- pack, beside a device-to-device copy of as many bytes ----
        pack_ms, copy_ms, index = [], [], None
        for rep in range(args.repeats + 1):  # (the first is the warm-up: the table pool of the context)
            w = ArchiveWriter(ctx)
            ctx.sync()
            t0 = time.perf_counter()
            w.append(arena, offs0, sizes0, body[:n0], dst_capacity=n0)
            w.append(tail, offs1, sizes1, body[n0:], dst_capacity=n1)
            ctx.sync()
            t1 = time.perf_counter()
            index = w.finish(si, vi)
            w.close()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            twin.copy_(body)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if rep:
                pack_ms.append(round((t1 - t0) * 1e3, 3))
                copy_ms.append(round((t3 - t2) * 1e3, 3))
        gbps = lambda ms: round((n0 + n1) / (float(np.median(ms)) * 1e-3) / 1e9, 1)
        entry = {"blocks": int(res.blocks), "body_bytes": n0 + n1, "index_bytes": len(index),
                 "pack": {"k_archive_pack_ms": pack_ms, "torch_copy_ms": copy_ms, "k_archive_pack_GBps_median": gbps(pack_ms),
                          "torch_copy_GBps_median": gbps(copy_ms)}}
        # ---- restore from the body, beside the restore from the aligned images ----
        a = Archive(index, n0 + n1, lib)
        offsets, out_bytes = Restore.layout(a.version_index, 1, lib)
        assert out_bytes == n
        entry["image_offset_residues_mod_8"] = sorted(set(int(o) % 8 for o in a.block_offsets))
        scratch = None
        for verify in (False, True):
            ms = {"archive": [], "aligned": []}
            for rep in range(args.repeats + 1):
                for kind in ("archive", "aligned"):
                    out.fill_(0xA5)
                    rs = Restore(ctx, a.version_index, a.store_index, offsets, n, verify=verify)
                    if scratch is None:
                        scratch = torch.empty(max(64, rs.archive_scratch_bound(a, 0, n0 + n1)), **u8)
                    ctx.sync()
                    t0 = time.perf_counter()
                    if kind == "archive":
                        delivered, nxt = rs.archive_blocks(a, body, 0, scratch, out)
                        assert delivered == res.blocks and nxt == n0 + n1
                    else:
                        for images, h, o, z in calls:
                            if len(h):
                                rs.blocks(h, images, o, z, scratch, out)
                    code, result = rs.finish()
                    t1 = time.perf_counter()
                    assert code == 0 and result.bytes_written == n, (code, result.bytes_written)
                    if rep == 0:
                        assert torch.equal(out, data[:n]), "the restored bytes differ from the tree"
                    else:
                        ms[kind].append(round((t1 - t0) * 1e3, 3))
                    rs.close()
            med = {k: float(np.median(v)) for k, v in ms.items()}
            entry["verify" if verify else "no_verify"] = {
                "from_the_archive_body_ms": ms["archive"], "from_aligned_images_ms": ms["aligned"],
                "from_the_archive_body_GBps_median": round(n / (med["archive"] * 1e-3) / 1e9, 1),
                "from_aligned_images_GBps_median": round(n / (med["aligned"] * 1e-3) / 1e9, 1),
                "archive_over_aligned": round(med["archive"] / med["aligned"], 3)}
        a.close()
        report["stores"][codec] = entry
        print(codec, json.dumps(entry), flush=True)
        del arena, tail, scratch, body, twin
    plan.close()
    ctx.close()
    path = Path(args.out)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
