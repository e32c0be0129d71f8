"""lz4_grid_rule.h (the launch grid of k_lz4_segments) compiled for the host as it stands, for tests/test_lz4_grid_rule.py and
tests/test_gpu_lz4_write_paths.py.  No GPU, no HIP: the header is plain C++."""
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "longtail_amd" / "csrc" / "lz4" / "lz4_grid_rule.h"
THREADS = 512      # a workgroup of k_lz4_segments: 64 * LZ4_G_BATCH
GROUP_UNITS = 8    # LZ4_G_BATCH
MAX_X, MAX_Y, MAX_THREADS = 0x7FFFFFFF, 65535, 0xFFFFFFFF  # gridDim.x, gridDim.y, threads of one launch

MAIN = r"""
#include <stdio.h>
#include "lz4_grid_rule.h"
int main()
{
    unsigned long long total;
    unsigned mx, blocks, threads;
    while (scanf("%llu %u %u %u", &total, &mx, &blocks, &threads) == 4)
    {
        const Lz4Grid g = lz4_grid_rule(total, mx, blocks, threads);
        printf("%u %u %d\n", g.x, g.y, (int)g.two_d);
    }
    return 0;
}
"""


def host_compiler():
    for name in ("c++", "g++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    return None


def build(directory: Path) -> Path:
    """-> the program: lines of `total_groups max_groups block_count threads` in, `x y two_d` out"""
    (directory / "rule.cpp").write_text(MAIN)
    res = subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(HEADER.parent), "-o", str(directory / "rule"),
                          str(directory / "rule.cpp")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return directory / "rule"


def ask(program: Path, cases):
    """cases: [(total_groups, max_groups, block_count, threads)] -> [(x, y, two_d)]"""
    text = "".join(f"{t} {m} {b} {th}\n" for t, m, b, th in cases)
    out = subprocess.run([str(program)], input=text, capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 3 * len(cases)
    return [(int(out[3 * i]), int(out[3 * i + 1]), bool(int(out[3 * i + 2]))) for i in range(len(cases))]


def groups_of(sizes, unit=4096):
    """the classification groups of every block of a batch (upload_blocks: ncgrp)"""
    return [((n + unit - 1) // unit + GROUP_UNITS - 1) // GROUP_UNITS for n in sizes]


def batch_case(sizes, unit=4096):
    g = groups_of(sizes, unit)
    return (sum(g), max(g, default=0), len(g), THREADS)
