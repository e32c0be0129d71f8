"""-m gpu: every BLAKE3 tree shape through each of the five reducers of k_blake3.hip, digest for digest against the oracle (which
tests/test_blake3_shapes_cases.py pins to the reference on the same tables).  Equality of the 64-bit digests, no tolerance.

  window   k_blake3_leaves + k_blake3_parents_window   hash_ranges(max_len <= 256 KiB), hash_runs_u64 with bounds, the fused chunk_hash
  level    k_blake3_parents_level + k_blake3_emit      hash_ranges(max_len = 0 or > 256 KiB), hash_runs_u64 without bounds
  one      k_blake3_one                                hash_one, from device and from pinned host memory
  stream   k_blake3_stream_batch / _final              b3_stream
  serial   k_blake3_parents_small                      the ablation build with LTHIP_B3_SERIAL_PARENTS

What a reducer has to get right for every leaf count n and tail t -- ROOT on the last merge or the single leaf, the odd node carried,
the chunk counter, the last block masked to its length -- is what the tables of tests/blake3_shapes.py walk.  Every output word is
preset to a sentinel, so a range no workgroup owns fails too.  A failure names (n, t, residue, position in the batch)."""
import ctypes as C
import errno

import numpy as np
import pytest
import torch

from tests import blake3_shapes as S
from tests.gpu_util import check_part, dev_u32, dev_u64, gpu_chunk_hash, u64

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def src(oracle):
    """(host bytes, the same on the device) every range call reads."""
    host = S.source(oracle)
    return host, torch.from_numpy(host).cuda()


@pytest.fixture(scope="module")
def expected(oracle, src):
    """The oracle's digests of a table, computed once per module."""
    memo = {}

    def get(name, table):
        if name not in memo:
            cases, offs, lens = table()
            memo[name] = (cases, offs, lens, oracle.blake3_many(src[0], offs, lens))
        return memo[name]

    return get


def sentinels(n):
    return torch.full((max(1, n),), SENTINEL, dtype=torch.int64, device="cuda")


def ranges(ctx, dev, offs, lens, max_len):
    out = sentinels(len(offs))
    ctx.hash_ranges(dev, dev_u64(offs), dev_u32(lens), max_len=max_len, out=out)
    return u64(out)[: len(offs)]


# ---- window reducer ----
@pytest.mark.parametrize("order", ["table", "reversed", "shuffled"])
def test_window_table(gpu, src, expected, order):
    """The whole N_SMALL table as one batch of 218 densely packed windows: every shape meets many positions inside a window."""
    cases, offs, lens, exp = expected("small", S.small_table)
    idx = np.arange(len(cases))
    if order == "reversed":
        idx = idx[::-1].copy()
    elif order == "shuffled":
        idx = np.random.default_rng(3).permutation(len(cases))
    got = ranges(gpu, src[1], offs[idx], lens[idx], S.WINDOW_MAX_LEN)
    assert not (msg := S.first_mismatch(got, exp[idx], cases, idx)), msg


@pytest.mark.parametrize("name", list(S.window_scenarios()))
def test_window_scenario(gpu, oracle, src, name):
    cases, offs, lens = S.batch(S.window_scenarios()[name])
    exp = oracle.blake3_many(src[0], offs, lens)
    got = ranges(gpu, src[1], offs, lens, S.WINDOW_MAX_LEN)
    assert not (msg := S.first_mismatch(got, exp, cases)), f"{name}: {msg}"


def runs(ctx, oracle, src, mode):
    """Every run set of the table through hash_runs_u64: mode 'exact' / 'doubled' bounds, or None for the unbounded call."""
    host, dev = src
    values = dev[: S.SRC_BYTES].view(torch.int64)
    for name, first in S.run_sets():
        n = len(first) - 1
        counts = np.diff(first)
        exp = oracle.blake3_many(host, 8 * first[:-1].astype(np.uint64), 8 * counts)
        k = {"exact": 1, "doubled": 2, None: 0}[mode]
        out = sentinels(n)
        if mode is None:
            ctx.hash_runs_u64(values, dev_u32(first), n, out=out)
        else:
            ctx.hash_runs_u64_bounded(values, dev_u32(first), n, k * int(first[-1]), k * int(counts.max()), out=out)
        cases = [(S.leaves(8 * int(c)), (8 * int(c) - 1) % S.KIB + 1 if c else 0, 0) for c in counts]
        assert not (msg := S.first_mismatch(u64(out)[:n], exp, cases)), f"run set {name}, bounds {mode}: {msg}"


@pytest.mark.parametrize("mode", ["exact", "doubled"])
def test_window_runs_bounded(gpu, oracle, src, mode):
    """Runs of 64-bit values with the caller's bounds: nothing is read back, the grid is sized by the bound.  Doubled, the leaf bound
    exceeds the total and the trailing windows are empty (set 'half'; the sets with runs of 256 KiB then lie above the window limit
    and take the level reducer, sized by the bound all the same)."""
    runs(gpu, oracle, src, mode)


# ---- the fused call: count on the device, leaf upper bound ----
@pytest.mark.parametrize("m", list(S.FUSED_M) + [S.FUSED_LEVEL[0]])
def test_fused_fixed_chunks(gpu, oracle, m):
    """(m, m, m): every chunk is m bytes and the last of a part the remainder -- 1, 2, 3, 4 and 65 leaves per chunk in thousands of
    equal trees; 300000 lies above the window limit: the level reducer with the count read back."""
    if m == S.FUSED_LEVEL[0]:
        sizes = [S.FUSED_LEVEL[1]]
    else:
        q = S.FUSED_M[m]
        sizes = [q * m, q * m + 1, q * m + m - 1]
    parts = [oracle.synth(s, 31 * m + i, 0) for i, s in enumerate(sizes)]
    for i, (got, data) in enumerate(zip(gpu_chunk_hash(gpu, parts, m, m, m), parts)):
        check_part(oracle, data, got, m, m, m,
                   what=f"(n={S.leaves(m)}, t={(m - 1) % S.KIB + 1}, residue=chunk index * {m} mod 4, part {i} of {len(data)} bytes)")


# ---- level reducer ----
@pytest.mark.parametrize("bound", ["unknown", "just_above_the_window_limit", "largest_length"])
def test_level_table(gpu, src, expected, bound):
    cases, offs, lens, exp = expected("level", S.level_table)
    idx = np.arange(len(cases))
    if bound == "unknown":
        max_len = 0  # the deepest tree a 32-bit length can have: 22 levels
    elif bound == "just_above_the_window_limit":
        max_len = S.WINDOW_MAX_LEN + 1
        idx = idx[lens <= max_len]  # up to (n=257, t=1): the level of stride 256 has one merge
        assert int(lens[idx].max()) == max_len
    else:
        max_len = int(lens.max())  # the stride loop ends exactly at ceil(max_len / 1024) = 4097 leaves
        assert S.leaves(max_len) == 4097
    got = ranges(gpu, src[1], offs[idx], lens[idx], max_len)
    assert not (msg := S.first_mismatch(got, exp[idx], cases, idx)), f"max_len={max_len}: {msg}"


def test_level_runs_unbounded(gpu, oracle, src):
    runs(gpu, oracle, src, None)


# ---- one-wave reducer ----
def one_calls(ctx, data, out, cases, offs, lens):
    for i in range(len(cases)):
        ctx.hash_one(data[int(offs[i]) :], int(lens[i]), out[i:])
    ctx.sync()


def test_one_device(gpu, src, expected):
    """1..64 leaves x every tail, and lengths 0 and 65536, at five residues mod 16 (vector staging at 0, byte staging elsewhere; dynamic
    LDS above 64 KiB from 62 leaves on): all calls queued into one digest tensor, read back once."""
    cases, offs, lens, exp = expected("one", S.one_table)
    out = sentinels(len(cases))
    one_calls(gpu, src[1], out, cases, offs, lens)
    assert not (msg := S.first_mismatch(u64(out), exp, cases)), msg


def test_one_pinned(gpu, src, oracle):
    """The same from pinned host memory (lthip_malloc_pinned), which is what the plugin layer hands the call."""
    cases, offs, lens = S.one_table(S.ONE_PINNED_RESIDUES)
    exp = oracle.blake3_many(src[0], offs, lens)
    dll, nbytes = gpu.lib.dll, len(src[0])
    p_in, p_out = C.c_void_p(), C.c_void_p()
    assert dll.lthip_malloc_pinned(gpu.h, nbytes, C.byref(p_in)) == 0
    try:
        assert dll.lthip_malloc_pinned(gpu.h, 8 * len(cases), C.byref(p_out)) == 0
        try:
            data = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p_in.value))
            out = np.ctypeslib.as_array((C.c_uint64 * len(cases)).from_address(p_out.value))
            data[:] = src[0]
            out[:] = SENTINEL
            one_calls(gpu, data, out, cases, offs, lens)
            got = out.copy()
        finally:
            gpu.sync()
            dll.lthip_free_pinned(gpu.h, p_out)
    finally:
        gpu.sync()
        dll.lthip_free_pinned(gpu.h, p_in)
    assert not (msg := S.first_mismatch(got, exp, cases)), msg


def test_one_above_64k_is_einval(gpu, src):
    out = sentinels(1)
    assert gpu.lib.dll.lthip_hash_one(gpu.h, src[1].data_ptr(), 65537, out.data_ptr()) == errno.EINVAL
    gpu.sync()
    assert int(u64(out)[0]) == SENTINEL


# ---- stream reducer ----
def test_stream(gpu, oracle):
    """B batches of 1 MiB and a tail: every depth of the subtree stack up to 4 below the tail, every merge count after a batch, tails
    of 1 .. 8 leaves and of a whole batch, the empty stream."""
    host = oracle.synth(S.STREAM_BYTES, S.SRC_SEED + 1, S.SRC_KIND)
    dev = torch.from_numpy(host).cuda()
    for i, (B, tail) in enumerate(S.stream_cases()):
        n = B * S.STREAM_BATCH + tail
        got, exp = gpu.b3_stream(dev, n), oracle.blake3(host[:n])
        assert got == exp, (f"(B={B}, tail={tail}: n={S.leaves(n)}, t={(tail - 1) % S.KIB + 1 if tail else 0}, residue=0, case {i}): "
                            f"got {got:016x}, expected {exp:016x}")


# ---- the serial reducer of the ablation build ----
def test_serial_parents_table(gpu_abl, src, expected, monkeypatch):
    monkeypatch.setenv("LTHIP_B3_SERIAL_PARENTS", "1")
    gpu_abl.lib.dll.lthip_debug_reload_env()
    cases, offs, lens, exp = expected("small", S.small_table)
    got = ranges(gpu_abl, src[1], offs, lens, S.WINDOW_MAX_LEN)
    assert not (msg := S.first_mismatch(got, exp, cases)), msg
