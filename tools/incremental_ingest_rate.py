#!/usr/bin/env python3
"""Ingest against a store that already has content: ONE synthetic tree resident in HBM, run through the stream session
(lthip_chunk_hash + lthip_ingest_stream_slice per slice, then finish) with

  no store    what the session did before it could consult one: every version-unique chunk is compressed and written
  50 / 90 / 100 %   an lthip_store attached that holds about that share of the version's unique chunks, taken by hash value (the low
              bits of the hash), so that the known chunks scatter over the tree and the written ones leave holes

Recorded into profiles/incremental_ingest_rate.json, per case: ms per step of every repeat and their median, GB/s of input, chunks and
blocks written, the share of the written blocks that went through the block assembly (gather), the share of the unique chunks the
store held; and, on their own, the time of lthip_store_find over all chunks of the version and of building a store of 10x the
version's chunks (created for that many / grown from 1024 slots in ten adds).  `no_store_spread_ms` is max - min of the no-store
repeats: what a difference between two cases has to exceed to mean anything.  There is no threshold.

A step is timed from the host, stream idle to stream idle; the session is created, fed and finished inside the timed region, the store
is built outside it (its cost is reported separately).

    python tools/incremental_ingest_rate.py [--gib 4] [--slices 4] [--repeats 5] [--out profiles/incremental_ingest_rate.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kind", default="mixed")
    ap.add_argument("--target-chunk-size", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=8 << 20)
    ap.add_argument("--max-chunks-per-block", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "incremental_ingest_rate.json"))
    args = ap.parse_args()

    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Context, Ingest, IngestStream, Store, chunker_params, load

    lib = load()
    dev = torch.device("cuda", 0)
    ctx = Context(0, lib=lib)
    S = args.slices
    nfiles = int(args.gib * (1 << 30)) // FILE // S  # per slice
    n = nfiles * FILE
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE)
    p_size = np.full(nfiles, FILE, np.uint64)
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)
    cap = max(1, plan.capacity)
    whole_tree = make_tree("files", S * n, FILE)
    whole, _keep_whole = Ingest.tree(whole_tree["sizes"], whole_tree["path_offsets"], whole_tree["perms"], whole_tree["path_data"],
                                     np.arange(S * nfiles, dtype=np.uint32), np.zeros(S * nfiles + 1, np.uint64))

    def session():
        return IngestStream(ctx, whole, args.target_chunk_size, args.block_size, args.max_chunks_per_block, "lz4")

    probe = session()
    arena_bytes, tail_arena_bytes = probe.arena_bound(n, cap), probe.arena_bound(0, 0)
    probe.close()

    u8 = dict(dtype=torch.uint8)
    data = [torch.empty(n + 256, device=dev, **u8) for _ in range(S)]  # the tree, resident
    for k in range(S):
        ctx.synth_fill(data[k], p_off, p_size, asset_seeds(0x10C0FFEE, k * nfiles, nfiles), KINDS[args.kind])
    ctx.sync()
    arena = torch.empty(arena_bytes, device=dev, **u8)
    tail_arena = torch.empty(tail_arena_bytes, device=dev, **u8)
    outs = (torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
            torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(nfiles + 1, dtype=torch.int32, device=dev))
    vi_cap = int(lib.dll.lthip_version_index_size(S * nfiles, S * cap, S * cap, len(whole_tree["path_data"]))) + 64
    h_vi, h_si = torch.empty(vi_cap, **u8).pin_memory(), torch.empty(16 + 32 * S * cap + 64, **u8).pin_memory()

    # ---- the version's chunk hashes, once: what the stores are drawn from ----
    every = []
    for k in range(S):
        total, _, _, d_hash, _ = ctx.chunk_hash(plan, data[k], outputs=outs)
        every.append(d_hash[:total].clone())
    all_hashes = torch.cat(every)
    unique = torch.unique(all_hashes)
    del every

    def store_with(percent):
        """about `percent` of the unique chunks, by the low ten bits of the hash"""
        held = unique[(unique & 1023) < (1024 * percent) // 100]
        store = Store(ctx, int(held.numel()))
        store.add(held)
        store.sync()
        return store, int(held.numel())

    def step(store):
        """-> (seconds, result, known chunks)"""
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        st = session()
        if store is not None:
            st.set_store(store)
        for k in range(S):
            total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, data[k], outputs=outs)
            st.slice(k * nfiles, nfiles, data[k], d_off, d_len, d_hash, d_first, total, arena)
            st.images()  # (the arena is reused by the next slice: a null sink)
        res = st.finish(tail_arena, h_vi, h_si)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        known = st.store_stats()[0]
        st.close()
        return dt, res, known

    report = {"workload": f"{S * n / (1 << 30):g} GiB ({S * nfiles} '{args.kind}' files of 1 MiB) resident in HBM, stream session in {S} slices, LZ4, "
                          f"target chunk {args.target_chunk_size}, blocks of {args.block_size} bytes / {args.max_chunks_per_block} chunks",
              "unit": "ms per step (lthip_chunk_hash + lthip_ingest_stream_slice per slice, finish), host clock, stream idle to stream idle",
              "repeats": args.repeats, "chunks": int(all_hashes.numel()), "unique_chunks": int(unique.numel()), "cases": {}}
    for name, percent in (("no store", None), ("50 %", 50), ("90 %", 90), ("100 %", 100)):
        store, held = store_with(percent) if percent is not None else (None, 0)
        step(store)  # warm-up: workspaces of the context, the plan
        runs = [step(store) for _ in range(args.repeats)]
        ms = [round(r[0] * 1e3, 3) for r in runs]
        res, known = runs[-1][1], runs[-1][2]
        entry = {"ms": ms, "ms_median": float(np.median(ms)), "GBps_input_median": round(S * n / (float(np.median(ms)) * 1e-3) / 1e9, 1),
                 "store_hashes": held, "known_share_of_unique_chunks": round(known / max(1, res.unique_all), 4),
                 "chunks_written": int(res.unique_local), "raw_bytes_written": int(res.raw_bytes), "compressed_bytes": int(res.compressed_bytes),
                 "blocks_written": int(res.blocks), "gathered_share_of_blocks": round(res.gathered_blocks / max(1, res.blocks), 4)}
        report["cases"][name] = entry
        print(name, json.dumps(entry), flush=True)
        if store is not None:
            store.close()
    base = report["cases"]["no store"]["ms"]
    report["no_store_spread_ms"] = round(max(base) - min(base), 3)

    # ---- the store's own calls ----
    def timed(fn, repeats):
        out = []
        for _ in range(repeats):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append(round((time.perf_counter() - t0) * 1e3, 3))
        return out

    store, _ = store_with(90)
    store.find(all_hashes)
    report["store_find_ms"] = {"queries": int(all_hashes.numel()), "ms": timed(lambda: store.find(all_hashes), args.repeats)}
    store.close()
    big = 10 * int(all_hashes.numel())
    many = torch.randint(-(2**62), 2**62, (big,), dtype=torch.int64, device=dev)
    pieces = many.chunk(10)

    def build(expected):
        s = Store(ctx, expected)
        for p in pieces:
            s.add(p)
        s.sync()
        grown = s.grown
        s.close()
        return grown

    report["store_build_10x_ms"] = {"hashes": big, "created_for_them": timed(lambda: build(big), 3), "grown_from_1024_slots": timed(lambda: build(0), 3),
                                    "growths": build(0)}
    print("store", json.dumps({k: report[k] for k in ("store_find_ms", "store_build_10x_ms", "no_store_spread_ms")}), flush=True)
    plan.close()
    ctx.close()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
