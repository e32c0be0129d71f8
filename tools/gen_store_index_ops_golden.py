#!/usr/bin/env python3
"""Generates tests/golden/store_index_ops_ref.npz from the REFERENCE (run in the build container only; needs
oracle/_ref/liblongtail_ref.so).  The output is DATA: for every case of tests/store_index_ops_util.py what Longtail_MergeStoreIndex /
Longtail_PruneStoreIndex followed by Longtail_WriteStoreIndexToBuffer gave,
  <op>/out/<case>  the serialized StoreIndex (uint8), or
  <op>/err/<case>  the errno (int32) of a call the reference refused.
tests/test_store_index_ops_abi.py compares the library with it on machines without the reference."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests._libs import ref  # noqa: E402
from tests.store_index_ops_util import GOLDEN_FILE, MERGES, PRUNES, RefOps  # noqa: E402


def main():
    r = RefOps(ref())
    table = {}
    for op, cases, call in (("merge", MERGES, r.merge), ("prune", PRUNES, r.prune)):
        for name, args in cases.items():
            got = call(*args)
            if isinstance(got, bytes):
                table[f"{op}/out/{name}"] = np.frombuffer(got, np.uint8)
            else:
                table[f"{op}/err/{name}"] = np.int32(got)
    np.savez_compressed(GOLDEN_FILE, **table)
    print(f"{GOLDEN_FILE}: {len(table)} results, {GOLDEN_FILE.stat().st_size} bytes")


if __name__ == "__main__":
    main()
