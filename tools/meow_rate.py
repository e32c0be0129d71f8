#!/usr/bin/env python3
"""Rates of the Meow ('meow') kernels on one GPU, printed as one JSON line:
  ranges   lthip_meow_ranges over the chunks of a resident slice of random 1 MiB files (HPCDC at --target), GB/s of chunk bytes,
           beside lthip_blake2s_ranges and lthip_hash_ranges (BLAKE3) over the same chunks
  chain    one long serial chain: us per MiB of lthip_meow_one (64 KiB, device memory), of lthip_meow_runs_u64 (one run of 2^20
           values = 8 MiB) and of the stream pair (8 MiB in 1 MiB batches)
  drop_in  Longtail_CreateVersionIndex of the reference core (oracle/_ref, when built) over a 1 GiB tree at --workers, HIP chunker
           with the HIP BLAKE3 object and with the HIP Meow object (its per-window digest table), GB/s
usage: tools/meow_rate.py [--gib 8] [--target 65536] [--reps 5] [--workers 16]"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from longtail_amd.lib import Context, chunker_params  # noqa: E402
from tools.blake2_rate import timed  # noqa: E402


def drop_in(ctx, workers):
    from tests._libs import have_ref, ref

    if not have_ref():
        return {}
    r = ref()
    lib = ctx.lib.dll
    files = [(f"d{i % 4}/f{i:03d}.bin", np.random.default_rng(100 + i).integers(0, 256, size=32 << 20, dtype=np.uint8)) for i in range(32)]
    total = sum(len(d) for _, d in files)
    out = {}
    for name, make in (("blake3", lib.Longtail_CreateHipBlake3HashAPI), ("meow", lib.Longtail_CreateHipMeowHashAPI)):
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
    ap.add_argument("--gib", type=float, default=8.0)
    ap.add_argument("--target", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
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
    tm = timed(lambda: ctx.meow_ranges(data, d_off, d_len, mx, out=out), a.reps)
    t2 = timed(lambda: ctx.blake2s_ranges(data, d_off, d_len, mx, out=out), a.reps)
    t3 = timed(lambda: ctx.hash_ranges(data, d_off, d_len, mx, out=out), a.reps)
    one_in = torch.randint(0, 256, (65536,), dtype=torch.uint8, device="cuda")
    one_out = torch.empty(1, dtype=torch.int64, device="cuda")
    t_one = timed(lambda: ctx.meow_one(one_in, 65536, one_out), a.reps)
    vals = torch.randint(0, 2**62, (1 << 20,), dtype=torch.int64, device="cuda")
    first = torch.tensor([0, 1 << 20], dtype=torch.int32, device="cuda")
    t_run = timed(lambda: ctx.meow_runs_u64(vals, first, 1), a.reps)
    t_stream = timed(lambda: ctx.meow_stream(vals, 8 << 20), a.reps)
    res = dict(gib=a.gib, target=a.target, chunks=total, chunk_bytes=nbytes,
               meow_ranges_ms=tm * 1e3, meow_ranges_gbps=nbytes / tm / 1e9,
               blake2s_ranges_ms=t2 * 1e3, blake2s_ranges_gbps=nbytes / t2 / 1e9,
               blake3_ranges_ms=t3 * 1e3, blake3_ranges_gbps=nbytes / t3 / 1e9,
               meow_one_64k_us=t_one * 1e6, meow_one_us_per_mib=t_one * 1e6 * 16,
               meow_runs_8mib_ms=t_run * 1e3, meow_runs_us_per_mib=t_run * 1e6 / 8,
               meow_stream_8mib_ms=t_stream * 1e3, meow_stream_us_per_mib=t_stream * 1e6 / 8)
    res.update(drop_in(ctx, a.workers))
    print(json.dumps(res))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
