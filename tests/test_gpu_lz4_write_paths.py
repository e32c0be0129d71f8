"""-m gpu: the write pass's short paths (k_lz4.hip).  A block none of whose units holds a sequence is laid out by the match finder and
skips the stitch's walk (k_lz4_stitch_scan reads the block's count of units with a sequence); the classification pass finds a
workgroup's block from a two-dimensional grid where the batch's blocks are about equally long, by bisection elsewhere
(lz4_grid_rule.h).  Neither may change a byte:
  1  all-literal blocks of every length around the format's and the parser's boundaries are the literal run built here in numpy
  2  a batch of about equal blocks (two-dimensional grid) that interleaves all-literal blocks with zeros, "mixed" data and random
     blocks with ONE planted 64-byte repeat -- in the first unit, in the last, across a 32 KiB half boundary, across a 64 KiB group
     boundary: every payload is the one the block has alone in a call, and decodes to its source
  3  one 1 MiB block among 3000 blocks of 64 bytes (one-dimensional grid): the same; and the rule says which grid either batch took
  4  a window one byte too small, for an all-literal block and for one with matches: size 0, the neighbours as they are alone,
     no byte outside any window (every call here runs on guarded windows, on two fills)
  5  the batch of 2 through zstd_compress_blocks    6  ... and with 1 KiB units (the batch parser's geometry for everything)"""
import numpy as np
import pytest

from tests import codec_windows_util as W
from tests import lz4_grid_rule_host as H
from tests._libs import have_ref, ref as get_ref

pytestmark = pytest.mark.gpu


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def planted(n, seed, src, dst):
    """noise with the 64 bytes at `src` repeated at `dst`"""
    d = noise(n, seed)
    d[dst : dst + 64] = d[src : src + 64]
    return d


N = 150000  # 37 units: 5 classification groups, 3 groups of the lane parser
LAST = (N // 4096) * 4096  # the last unit's start


def mixture(oracle):
    """[(name, bytes)]: about equal lengths (5 classification groups each, but for one short and one empty block)"""
    return [("noise a", noise(N, 1)), ("zeros", np.zeros(160000, np.uint8)), ("noise b", noise(163840, 2)),
            ("repeat in the first unit", planted(N, 3, 16, 100)), ("mixed a", oracle.synth(155000, 7, 1)), ("noise c", noise(N + 1, 4)),
            ("repeat in the last unit", planted(N, 5, LAST + 16, LAST + 100)), ("empty", np.zeros(0, np.uint8)), ("noise d", noise(4097, 6)),
            ("repeat across a 32 KiB half boundary", planted(N, 8, 32768 - 232, 32768 - 32)), ("mixed b", oracle.synth(140000, 9, 1)),
            ("repeat across a 64 KiB group boundary", planted(N, 10, 65536 - 232, 65536 - 32)), ("noise e", noise(N, 11))]


def residue(i):
    return (3 * i + 1) % 16  # (a block keeps its source residue in every call: the parse may depend on the source's alignment)


def encode(call, datas, bound, residues, caps=None):
    """one call on guarded windows, on two fills -> (sizes, windows); no byte outside a window, both fills agree"""
    caps = caps or [bound(len(d)) for d in datas]
    lay = W.build_layout(list(datas), [(residues[i], (2 * i + 1) % 16, caps[i]) for i in range(len(datas))], "guarded")
    first, second = W.run(lay, call)
    W.check_guards(lay, (first, second))
    assert (first.sizes == second.sizes).all()
    for b in range(len(datas)):
        s = int(first.sizes[b])
        assert s <= caps[b] and (first.windows[b][:s] == second.windows[b][:s]).all(), lay.describe(b)
    return [int(s) for s in first.sizes], [w.copy() for w in first.windows]


def payloads(call, datas, bound, residues):
    sizes, windows = encode(call, datas, bound, residues)
    assert all(s > 0 for s in sizes), sizes
    return [w[:s] for s, w in zip(sizes, windows)]


def decodes(call, pays, datas):
    """every payload back to its source through a decoder of this library, one call"""
    lay = W.build_layout(pays, [(i % 16, (2 * i + 1) % 16, len(d)) for i, d in enumerate(datas)], "guarded")
    results = W.run(lay, call)
    W.check_guards(lay, results)
    for res in results:
        for b, d in enumerate(datas):
            assert int(res.sizes[b]) == len(d) and (res.windows[b] == d).all(), f"block {b} ({len(d)} bytes) decodes to {int(res.sizes[b])}"


def same(got, want, names, what):
    bad = [f"'{n}': {len(g)} bytes against {len(w)} alone" for n, g, w in zip(names, got, want) if len(g) != len(w) or not (g == w).all()]
    assert not bad, f"{what}: {len(bad)} payloads are not the ones the blocks have alone, the first: " + "; ".join(bad[:8])


_alone = {}


def alone(key, call, datas, bound, residues):
    """every block in a call of its own, once per module"""
    if key not in _alone:
        _alone[key] = [payloads(call, [d], bound, [residues[i]])[0] for i, d in enumerate(datas)]
    return _alone[key]


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    program = H.build(tmp_path_factory.mktemp("lz4grid"))
    return lambda sizes: H.ask(program, [H.batch_case(sizes)])[0]


def literal_run(d):
    n = len(d)
    head = [n << 4] if n < 15 else [0xF0] + [255] * ((n - 15) // 255) + [(n - 15) % 255]
    return np.concatenate([np.asarray(head, np.uint8), d])


def test_all_literal_blocks(gpu):
    sizes = [1, 11, 12, 13, 4095, 4096, 4097, 32767, 32768, 32769, 65541, 300000]
    datas = [noise(n, 100 + i) for i, n in enumerate(sizes)]
    pays = payloads(gpu.lz4_compress_blocks, datas, W.lz4_bound, [residue(i) for i in range(len(datas))])
    for d, p in zip(datas, pays):
        want = literal_run(d)
        assert len(p) == len(want) == W.lz4_literal_run_size(len(d)) and (p == want).all(), f"{len(d)} bytes: {len(p)} against {len(want)}"
    decodes(gpu.lz4_decompress_blocks, pays, datas)
    if have_ref():
        r = get_ref()
        for d, p in zip(datas, pays):
            err, out = r.decompress(0, p, len(d))
            assert err == 0 and len(out) == len(d) and (out == d).all(), f"{len(d)} bytes: the reference decodes with error {err}"


def test_mixed_batch(gpu, oracle, rule):
    names, datas = zip(*mixture(oracle))
    res = [residue(i) for i in range(len(datas))]
    assert rule([len(d) for d in datas])[2], "this batch is meant for the two-dimensional grid"
    want = alone("lz4", gpu.lz4_compress_blocks, datas, W.lz4_bound, res)
    got = payloads(gpu.lz4_compress_blocks, datas, W.lz4_bound, res)
    for n, d, p in zip(names, datas, got):
        print(f"lz4 write paths, '{n}': {len(d)} -> {len(p)} bytes (a literal run: {W.lz4_literal_run_size(len(d))})")
    same(got, want, names, "mixed batch")
    for n, d, p in zip(names, datas, got):  # (both routes are in the batch)
        if n.startswith("noise"):
            assert len(p) == W.lz4_literal_run_size(len(d)), n
        elif n.startswith(("zeros", "mixed")):
            assert len(p) < len(d), n
    decodes(gpu.lz4_decompress_blocks, got, datas)


def test_skewed_batch(gpu, oracle, rule):
    tiny = [noise(64, 20), np.zeros(64, np.uint8), noise(64, 21), np.tile(np.arange(8, dtype=np.uint8), 8), noise(64, 22),
            np.concatenate([noise(32, 23)] * 2), noise(64, 24), np.full(64, 7, np.uint8)]
    long_block = np.concatenate([oracle.synth(1 << 19, 31, 1), noise(1 << 19, 32)])
    datas = [long_block] + [tiny[i % 8] for i in range(3000)]
    res = [5] + [i % 16 for i in range(3000)]
    assert rule([len(d) for d in datas]) == (sum(H.groups_of([len(d) for d in datas])), 1, False), "this batch is meant for the one-dimensional grid"
    # (a tiny block's content and residue repeat every 16 blocks: 17 calls give every block's payload alone)
    first = alone("skew", gpu.lz4_compress_blocks, datas[:17], W.lz4_bound, res[:17])
    want = [first[0]] + [first[1 + i % 16] for i in range(3000)]
    got = payloads(gpu.lz4_compress_blocks, datas, W.lz4_bound, res)
    same(got, want, ["the 1 MiB block"] + [f"tiny {i}" for i in range(3000)], "skewed batch")
    assert len(got[0]) < len(long_block)
    decodes(gpu.lz4_decompress_blocks, got, datas)


def test_a_window_one_byte_too_small(gpu, oracle):
    names, datas = zip(*mixture(oracle))
    res = [residue(i) for i in range(len(datas))]
    want = alone("lz4", gpu.lz4_compress_blocks, datas, W.lz4_bound, res)
    short = {names.index("noise c"): "all-literal", names.index("mixed a"): "with matches"}
    assert len(want[names.index("noise c")]) == W.lz4_literal_run_size(N + 1) and len(want[names.index("mixed a")]) < 155000
    caps = [len(want[i]) - 1 if i in short else W.lz4_bound(len(d)) for i, d in enumerate(datas)]
    sizes, windows = encode(gpu.lz4_compress_blocks, datas, W.lz4_bound, res, caps)
    for i, why in short.items():
        assert sizes[i] == 0, f"'{names[i]}' ({why}) in a window of {caps[i]} bytes: size {sizes[i]}"
    keep = [i for i in range(len(datas)) if i not in short]
    same([windows[i][: sizes[i]] for i in keep], [want[i] for i in keep], [names[i] for i in keep], "beside a block that does not fit")


def test_zstd_path(gpu, oracle):
    names, datas = zip(*mixture(oracle))
    res = [residue(i) for i in range(len(datas))]
    want = alone("zstd", gpu.zstd_compress_blocks, datas, W.zstd_bound, res)
    got = payloads(gpu.zstd_compress_blocks, datas, W.zstd_bound, res)
    same(got, want, names, "zstd")
    decodes(gpu.zstd_decompress_blocks, got, datas)


def test_without_speculative_placement_every_block_is_walked(gpu, gpu_abl, oracle, monkeypatch):
    """LTHIP_LZ4_DBG bit 6 (ablation build): no unit's bytes are placed by the match finder, so no block may skip the walk -- the copy
    kernel places every block from its plan.  The product's bytes."""
    names, datas = zip(*mixture(oracle))
    res = [residue(i) for i in range(len(datas))]
    want = alone("lz4", gpu.lz4_compress_blocks, datas, W.lz4_bound, res)
    monkeypatch.setenv("LTHIP_LZ4_DBG", "64")
    gpu_abl.lib.dll.lthip_debug_reload_env()
    got = payloads(gpu_abl.lz4_compress_blocks, datas, W.lz4_bound, res)
    monkeypatch.delenv("LTHIP_LZ4_DBG")
    gpu_abl.lib.dll.lthip_debug_reload_env()
    same(got, want, names, "no speculative placement")


def test_unit_size_1_kib(gpu, oracle):
    names, datas = zip(*mixture(oracle))
    res = [residue(i) for i in range(len(datas))]
    got = payloads(lambda *a: gpu.lz4_compress_blocks(*a, segment_log2=10), datas, W.lz4_bound, res)
    for n, d, p in zip(names, datas, got):
        if n.startswith(("zeros", "mixed")):
            assert len(p) < len(d), n
    decodes(gpu.lz4_decompress_blocks, got, datas)
