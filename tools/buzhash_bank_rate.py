#!/usr/bin/env python3
"""What adversarial bytes cost the Buzhash scans: lthip_chunk_hash over --gib of 1 MiB files (the walking scan that hashes, HPCDC at
--target), timed on random bytes and on bytes drawn from the eight values c, c + 32, ..., c + 224 -- one bank of the LDS table of
rotations (k_buzhash.hip), the worst conflict pattern a look-up can meet -- and printed as one JSON line.  LTHIP_LIB_PATH chooses the
library, so two builds are compared by running the tool once for each.
usage: tools/buzhash_bank_rate.py [--gib 4] [--target 65536] [--reps 5] [--bank 0]"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from longtail_amd.lib import Context, chunker_params  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--target", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bank", type=int, default=0)
    a = ap.parse_args()
    ctx = Context(0)
    size = 1 << 20
    nfiles = int(a.gib * 1024)
    offs, sizes = [i * size for i in range(nfiles)], [size] * nfiles
    mn, av, mx = chunker_params(a.target)
    plan = ctx.make_plan(offs, sizes, mn, av, mx)
    res = dict(gib=a.gib, target=a.target, bank=a.bank, walked_scans=plan.walked_scans, slices=plan.slices, build_id=ctx.lib.build_id())
    gen = torch.Generator(device="cuda").manual_seed(20261021)
    data = torch.zeros(nfiles * size + 64, dtype=torch.uint8, device="cuda")
    for name in ("random", "one_bank"):
        body = data[: nfiles * size]
        if name == "random":
            body.random_(0, 256, generator=gen)
        else:
            body.random_(0, 8, generator=gen).mul_(32).add_(a.bank % 32)
        ctx.timing(True)
        ms, kern, chunks = [], [], 0
        for rep in range(a.reps + 1):  # (the first is the warm-up)
            ctx.timing_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            chunks = ctx.chunk_hash(plan, data)[0]
            torch.cuda.synchronize()
            if rep:
                ms.append((time.perf_counter() - t0) * 1e3)
                kern.append(float(ctx.timing_get()["buzhash"][0]))
        ctx.timing(False)
        ms.sort(), kern.sort()
        res[name] = dict(chunks=int(chunks), chunk_hash_ms_min=round(ms[0], 3), chunk_hash_ms_median=round(ms[len(ms) // 2], 3),
                         buzhash_kernel_ms_min=round(kern[0], 3), gbps=round(nfiles * size / (ms[len(ms) // 2] * 1e-3) / 1e9, 1))
    print(json.dumps(res))
    plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
