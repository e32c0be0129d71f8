#!/usr/bin/env python3
"""Writing uncompressed blocks: ONE tree of 1 MiB random files resident in HBM, chunked and hashed once, then the WRITE PHASE of the
one-shot session (lthip_ingest_write: every block's image into the arena) timed for

  raw    tag 0 / LTHIP_CODEC_NONE: BlockIndex + the chunks' bytes, copied by k_raw_copy (k_gather.hip)
  lz4    'lz42' / LTHIP_CODEC_LZ4 on the same tree: on random bytes the codec stores every block uncompressed too, but probes first
  d2d    hipMemcpyAsync device to device of the same byte count, in the same process: the device's own copy

Both sessions move N bytes in and N bytes out; the report gives ms and TB/s of read + write (2 N / time) for all three, the median of
the repeats after a warm-up run of each, the three alternating within a repeat.  Two things are expected and REPORTED, not asserted:
the raw write phase takes no longer than the LZ4 one, and it reaches at least 0.8 of the device-to-device copy (the share the LZ4
stitch copy reaches against profiles/r06_copy_rates.txt).

The write phase is timed from the host, stream idle to stream idle, around lthip_ingest_write alone; lthip_ingest_index before it and
lthip_ingest_finish after it are outside the timed region.

    python tools/raw_store_rate.py [--gib 8] [--repeats 5] [--out profiles/raw_store_rate.json]
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FILE = 1 << 20
LZ4_TAG = 0x6C7A3432


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-chunk-size", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=8 << 20)
    ap.add_argument("--max-chunks-per-block", type=int, default=1024)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "raw_store_rate.json"))
    args = ap.parse_args()

    import torch

    from bench import KINDS, asset_seeds, make_tree
    from longtail_amd.lib import Context, Ingest, chunker_params, load

    if not torch.cuda.is_available():
        sys.exit("tools/raw_store_rate.py measures on a GPU: none found")
    lib = load()
    dev = torch.device("cuda", 0)
    ctx = Context(0, lib=lib)
    nfiles = max(1, int(args.gib * (1 << 30)) // FILE)
    n = nfiles * FILE
    mn, av, mx = chunker_params(args.target_chunk_size)
    p_off = np.arange(nfiles, dtype=np.uint64) * np.uint64(FILE)
    p_size = np.full(nfiles, FILE, np.uint64)
    u8 = dict(dtype=torch.uint8)
    data = torch.empty(n + 256, device=dev, **u8)
    ctx.synth_fill(data, p_off, p_size, asset_seeds(0x10C0FFEE, 0, nfiles), KINDS["random"])
    plan = ctx.make_plan(p_off, p_size, mn, av, mx)
    total, d_off, d_len, d_hash, d_first = ctx.chunk_hash(plan, data)
    job_first = d_first.cpu().numpy().view(np.uint32).astype(np.uint64)[: nfiles + 1]
    t = make_tree("files", n, FILE)
    tree, _keep = Ingest.tree(t["sizes"], t["path_offsets"], t["perms"], t["path_data"], np.arange(nfiles, dtype=np.uint32), job_first)
    # every image slot of one batch: header + codec bound, rounded to 64 -- a block holds at least a chunk, LZ4's bound is n + n / 255 + 16
    arena = torch.empty(n + n // 255 + total * 192 + (64 << 20), device=dev, **u8)
    copy_dst = torch.empty(n, device=dev, **u8)
    h_si = torch.empty(16 + 32 * max(1, total) + 64, **u8).pin_memory()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream(dev).cuda_stream

    sessions = {"raw": Ingest(ctx, args.target_chunk_size, args.block_size, args.max_chunks_per_block, "none", compression_type=0),
                "lz4": Ingest(ctx, args.target_chunk_size, args.block_size, args.max_chunks_per_block, "lz4", compression_type=LZ4_TAG)}
    results = {}

    def write_phase(name):
        ing = sessions[name]
        ing.index(tree, d_hash, d_len, total, d_off, d_first, total, None)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        ing.write(data, arena)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        results[name] = ing.finish(h_si)
        return dt

    def d2d(_name):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        err = hip.hipMemcpyAsync(copy_dst.data_ptr(), data.data_ptr(), n, 3, stream)  # hipMemcpyDeviceToDevice
        torch.cuda.synchronize(dev)
        assert err == 0, err
        return time.perf_counter() - t0

    cases = {"raw": write_phase, "lz4": write_phase, "d2d": d2d}
    for name, fn in cases.items():  # warm-up: workspaces, code objects
        fn(name)
    ms = {name: [] for name in cases}
    for _ in range(args.repeats):  # the three alternate within a repeat
        for name, fn in cases.items():
            ms[name].append(round(fn(name) * 1e3, 3))
    for name in ("raw", "lz4"):
        r = results[name]
        assert r.raw_bytes == n and r.unique_local == total, "random files: nothing dedups"
    assert results["raw"].compressed_bytes == n and results["raw"].gathered_blocks == 0

    def entry(name):
        med = float(np.median(ms[name]))
        return {"ms": ms[name], "ms_median": med, "TBps_read_plus_write_median": round(2 * n / (med * 1e-3) / 1e12, 3)}

    report = {"workload": f"{n / (1 << 30):g} GiB ({nfiles} random files of 1 MiB) resident in HBM, {total} chunks (target {args.target_chunk_size}), "
                          f"{int(results['raw'].blocks)} blocks of {args.block_size} bytes / {args.max_chunks_per_block} chunks, one codec batch",
              "unit": "ms of the write phase (lthip_ingest_write alone; d2d: one hipMemcpyAsync), host clock, stream idle to stream idle; "
                      "TB/s counts the bytes read plus the bytes written, 2 N",
              "bytes": n, "repeats": args.repeats, "cases": {name: entry(name) for name in cases},
              "lz4_stored_bytes": int(results["lz4"].compressed_bytes)}
    raw, lz4, copy = (report["cases"][k]["ms_median"] for k in ("raw", "lz4", "d2d"))
    report["expectations"] = {"raw_no_longer_than_lz4": {"raw_over_lz4": round(raw / lz4, 3), "met": raw <= lz4},
                              "raw_at_least_0.8_of_d2d": {"d2d_over_raw": round(copy / raw, 3), "met": copy / raw >= 0.8}}
    print(json.dumps(report), flush=True)
    for s in sessions.values():
        s.close()
    plan.close()
    ctx.close()
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(report, indent=1) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
