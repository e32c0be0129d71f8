"""Tiles per chunk of the walking scan (k_buzhash_walk): GIB (default 16) of 1 MiB random parts with the headline's chunker parameters,
the walking scan forced, the 4 KiB wave-tiles it hashed read from the ablation build's counter (lthip_debug_walk_tiles) and set against the
tile scan's N / 4096.  The log goes to profiles/walk_scan_sweep.txt.
usage: python tools/ablations/k1_walk_tiles.py [gib]"""
import ctypes as C
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
os.environ.setdefault("LTHIP_LIB_PATH", str(ROOT / "build" / "ablations" / "liblongtail_hip.so"))  # (the switch and the counter live there)
os.environ["LTHIP_K1_WALK"] = "1"
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from bench import KINDS  # noqa: E402
from longtail_amd.lib import Context, chunker_params  # noqa: E402

gib = float(sys.argv[1]) if len(sys.argv) > 1 else 16.0
ctx = Context(0)
sz = 1 << 20
n = int(gib * 1024)
offs = [i * sz for i in range(n)]
data = torch.zeros(n * sz + 256, dtype=torch.uint8, device="cuda")
ctx.synth_fill(data, offs, [sz] * n, [1000 + i for i in range(n)], KINDS["random"])
plan = ctx.make_plan(offs, [sz] * n, *chunker_params(65536))
tiles = C.c_uint64(0)
assert ctx.lib.dll.lthip_debug_walk_tiles(C.byref(tiles)) == 0, "needs the ablation build"
total = ctx.chunk_hash(plan, data)[0]
assert ctx.lib.dll.lthip_debug_walk_tiles(C.byref(tiles)) == 0
print(f"walked scans {plan.walked_scans} of {plan.slices}; bytes {n * sz} chunks {total} tiles hashed {tiles.value} = {tiles.value / total:.3f} tiles per chunk "
      f"(the tile scan: {n * sz / 4096 / total:.3f}) = {tiles.value * 4096 / (n * sz):.4f} of the bytes")
