#!/usr/bin/env python3
"""Rates of a chain hash's kernels ('blk2': BLAKE2s-64, 'meow': Meow-64) on one GPU, printed as one JSON line:
  ranges   lthip_<kind>_ranges over the chunks of a resident slice of random 1 MiB files (HPCDC at --target), GB/s of chunk bytes,
           beside the other hash types over the same chunks (lthip_hash_ranges is BLAKE3)
  chain    one long serial chain: us per MiB of lthip_<kind>_one (64 KiB, device memory), of lthip_<kind>_runs_u64 (one run of 2^20
           values = 8 MiB) and of the stream pair (8 MiB in 1 MiB batches)
  cpu      'blk2' only: BLAKE2s-64 on the CPU, 16 threads over 64 KiB pieces: Python's hashlib.blake2s (the BLAKE2 reference
           implementation)
  drop_in  Longtail_CreateVersionIndex of the reference core (oracle/_ref, when built) over a 1 GiB tree at --workers, HIP chunker
           with the HIP BLAKE3 object and with the kind's HIP object (its per-window digest table), GB/s
usage: tools/hash_rate.py --kind blk2|meow [--gib 8] [--target 65536] [--reps 5] [--workers 16]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from longtail_amd.lib import Context, chunker_params  # noqa: E402

# kind -> (prefix of the Context methods and of the JSON keys, the stream method, the drop-in key, the HashAPI constructor)
KINDS = {"blk2": ("blake2s", "b2s_stream", "blake2", "Longtail_CreateHipBlake2HashAPI"),
         "meow": ("meow", "meow_stream", "meow", "Longtail_CreateHipMeowHashAPI")}


def timed(fn, reps):
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def cpu_rate(threads):
    import hashlib
    from concurrent.futures import ThreadPoolExecutor

    buf = np.random.default_rng(1).integers(0, 256, size=1 << 30, dtype=np.uint8).tobytes()
    mv = memoryview(buf)
    piece = 1 << 16

    def work(t):
        for o in range(t * piece, len(buf), threads * piece):
            hashlib.blake2s(mv[o : o + piece], digest_size=8).digest()

    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(work, range(threads)))
        dt = time.perf_counter() - t0
    return dict(cpu_threads=threads, cpu_blake2s_gbps=len(buf) / dt / 1e9)


def drop_in(ctx, workers, label, constructor):
    from tests._libs import have_ref, ref

    if not have_ref():
        return {}
    r = ref()
    lib = ctx.lib.dll
    files = [(f"d{i % 4}/f{i:03d}.bin", np.random.default_rng(100 + i).integers(0, 256, size=32 << 20, dtype=np.uint8)) for i in range(32)]
    total = sum(len(d) for _, d in files)
    out = {}
    for name, make in (("blake3", lib.Longtail_CreateHipBlake3HashAPI), (label, getattr(lib, constructor))):
        chunker, hasher = lib.Longtail_CreateHipChunkerAPI(), make()
        r.version_index(files, 65536, workers, r.lz4_type, chunker_api=chunker, hash_api=hasher)  # warm-up
        _, secs = r.version_index(files, 65536, workers, r.lz4_type, chunker_api=chunker, hash_api=hasher)  # CreateVersionIndex alone
        out[f"drop_in_version_index_{name}_gbps"] = total / secs / 1e9
        for p in (chunker, hasher):
            C.CFUNCTYPE(None, C.c_void_p)(C.cast(p, C.POINTER(C.c_void_p))[0])(p)
    out["drop_in_workers"] = workers
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=sorted(KINDS), required=True)
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--target", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--no-drop-in", action="store_true", help="the kernels' rates only (no CPU section, no reference core)")
    a = ap.parse_args()
    name, stream, label, constructor = KINDS[a.kind]
    ctx = Context(0)
    nfiles = int(a.gib * 1024)
    size = 1 << 20
    data = torch.empty(nfiles * size + 64, dtype=torch.uint8, device="cuda")
    offs = [i * size for i in range(nfiles)]
    ctx.synth_fill(data, offs, [size] * nfiles, list(range(1, nfiles + 1)), 0)  # kind 0: random bytes
    mn, av, mx = chunker_params(a.target)
    plan = ctx.make_plan(offs, [size] * nfiles, mn, av, mx)
    total, d_off, d_len, _, _ = ctx.chunk_hash(plan, data, want_hashes=False)
    d_off, d_len = d_off[:total], d_len[:total]
    nbytes = int(d_len.to(torch.int64).sum().item())
    out = torch.empty(total, dtype=torch.int64, device="cuda")
    res = dict(kind=a.kind, gib=a.gib, target=a.target, chunks=total, chunk_bytes=nbytes)
    ranges = [(name, getattr(ctx, name + "_ranges"))]
    ranges += [(n, getattr(ctx, n + "_ranges")) for n, _, _, _ in KINDS.values() if n != name] + [("blake3", ctx.hash_ranges)]
    for n, fn in ranges:
        t = timed(lambda: fn(data, d_off, d_len, mx, out=out), a.reps)
        res.update({f"{n}_ranges_ms": t * 1e3, f"{n}_ranges_gbps": nbytes / t / 1e9})
    one_in = torch.randint(0, 256, (65536,), dtype=torch.uint8, device="cuda")
    one_out = torch.empty(1, dtype=torch.int64, device="cuda")
    t_one = timed(lambda: getattr(ctx, name + "_one")(one_in, 65536, one_out), a.reps)
    vals = torch.randint(0, 2**62, (1 << 20,), dtype=torch.int64, device="cuda")
    first = torch.tensor([0, 1 << 20], dtype=torch.int32, device="cuda")
    t_run = timed(lambda: getattr(ctx, name + "_runs_u64")(vals, first, 1), a.reps)
    t_stream = timed(lambda: getattr(ctx, stream)(vals, 8 << 20), a.reps)
    res.update({f"{name}_one_64k_us": t_one * 1e6, f"{name}_one_us_per_mib": t_one * 1e6 * 16,
                f"{name}_runs_8mib_ms": t_run * 1e3, f"{name}_runs_us_per_mib": t_run * 1e6 / 8,
                f"{name}_stream_8mib_ms": t_stream * 1e3, f"{name}_stream_us_per_mib": t_stream * 1e6 / 8})
    if not a.no_drop_in:
        if a.kind == "blk2":
            res.update(cpu_rate(a.workers))
        res.update(drop_in(ctx, a.workers, label, constructor))
    res["build_id"] = ctx.lib.build_id()
    print(json.dumps(res))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
