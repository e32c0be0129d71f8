"""-m gpu: the hand-built LZ4 payloads of tests/lz4_format_payloads.py (every corner of the block format and of the decoders, and the near
misses one step outside) through lthip_lz4_decompress_blocks, every way the library has of decoding them:
  (a) the product library as called: the wave-per-block decoder (lz4_decode_one: batch path, one-sequence fast path, general path)
      for capacities below 2 * PD_UNIT, the block-parallel path (k_lz4_pd_*, k_lz4_po_trace, k_lz4_po_gather) above -- the large
      cases, and every small case again with a capacity of 2 * PD_UNIT;
  (b) - (d) the ablation build with LTHIP_LZ4_SERIAL_DECODER=1 (the large cases on the wave-per-block decoder too),
      LTHIP_LZ4_NO_BATCH_DECODE=1 (one sequence per step; alone and with the serial switch), LTHIP_LZ4_PLAIN_DECODER=1;
  (e) the large cases with an origin arena of 1 MiB (one block per group) and of 4096 MiB;
  (f) the int64_t instantiation of k_lz4_decode_lds: one block of the call has a capacity of 1 GiB.
What is expected comes from the CPU side alone (tests/test_lz4_format_cases.py proves it against the oracle and the reference): a valid
(payload, capacity) pair gives its size and the model's bytes, a refused one 0xFFFFFFFF.  Payloads lie at every source residue mod 16,
destination windows at odd offsets between guard bytes (tests/codec_windows_util.py), on two fills: nothing outside the windows is
written, whatever the verdict."""
import functools
import re

import numpy as np
import pytest
import torch

from tests import codec_windows_util as W
from tests import lz4_format as Z
from tests import lz4_format_payloads as P

pytestmark = pytest.mark.gpu


def entry(c, cap, verdict):
    """(case, destination capacity, expected bytes | None = refused)"""
    return c, cap, (P.built(c["name"])[1] if verdict == "valid" else None)


@functools.lru_cache(maxsize=None)
def groups():
    """SMALL: the wave-per-block decoder, whatever the payload; LARGE: the block-parallel path (every one of these payloads has 64 bytes
    and more); ON_PAR: the small cases with a capacity of 2 * PD_UNIT.  (Built on first use: the models take a second or two.)"""
    pairs = [entry(c, cap, v) for c, cap, v in P.pairs()]
    small = [e for e in pairs if e[1] < Z.PAR_MIN_CAP]
    large = [e for e in pairs if e[1] >= Z.PAR_MIN_CAP]
    return small, large, [entry(c, Z.PAR_MIN_CAP, v) for c, v in P.small_on_parallel()]


def layout_of(entries):
    payloads = [np.frombuffer(P.built(c["name"])[0], np.uint8) for c, _, _ in entries]
    specs = [(i % 16, (2 * i + 1) % 16, cap) for i, (_, cap, _) in enumerate(entries)]  # source residues 0, 1, .. 15, 0, ..; odd destinations
    lay = W.build_layout(payloads, specs, "guarded")
    assert {o % 16 for o in lay.src_offs} == set(range(min(16, len(entries)))) and all(o % 2 for o in lay.dst_offs)
    return lay


def decode(ctx, entries):
    """one call on a guarded layout, twice (two fills) -> per entry the bytes or None; asserts the guards and that both runs agree"""
    lay = layout_of(entries)
    first, second = W.run(lay, ctx.lz4_decompress_blocks)
    W.check_guards(lay, (first, second))
    out = []
    for b in range(len(entries)):
        s = int(first.sizes[b])
        assert s == int(second.sizes[b]), lay.describe(b)
        if s == W.REFUSED:
            out.append(None)
        else:
            assert s <= lay.caps[b], lay.describe(b)
            assert (first.windows[b][:s] == second.windows[b][:s]).all(), f"{lay.describe(b)}: the bytes depend on what the window held"
            out.append(first.windows[b][:s].tobytes())
    return out


def check(entries, got, way):
    for (c, cap, want), g in zip(entries, got):
        what = f"{way}: '{c['name']}' (capacity {cap}, payload of {len(P.built(c['name'])[0])})"
        if want is None:
            assert g is None, f"{what} was accepted ({len(g)} bytes)"
        else:
            assert g is not None, f"{what} was refused"
            assert len(g) == len(want), f"{what}: {len(g)} bytes for {len(want)}"
            assert g == want, f"{what}: bytes differ first at {next(i for i in range(len(g)) if g[i] != want[i])}"


def test_small_cases_product_library(gpu):
    """(a) the wave-per-block decoder; run before anything else of this file"""
    SMALL, LARGE, ON_PAR = groups()
    assert len(SMALL) > 450 and all(len(P.built(c["name"])[0]) >= Z.PAR_MIN_PAYLOAD for c, _, _ in LARGE)
    check(SMALL, decode(gpu, SMALL), "product")


def test_large_cases_product_library(gpu):
    """(a) the block-parallel path"""
    SMALL, LARGE, ON_PAR = groups()
    check(LARGE, decode(gpu, LARGE), "product, block-parallel")


def test_small_cases_on_the_block_parallel_path(gpu):
    """(a) every small case whose verdict a roomy capacity leaves alone, with a capacity of 2 * PD_UNIT: payloads of 64 bytes and more
    take the block-parallel path"""
    SMALL, LARGE, ON_PAR = groups()
    check(ON_PAR, decode(gpu, ON_PAR), "product, small cases with a capacity of 2 * PD_UNIT")


def switched(ctx, monkeypatch, switches, body):
    for name, value in switches:
        monkeypatch.setenv(name, value)
    ctx.lib.dll.lthip_debug_reload_env()  # (the library caches its switches)
    try:
        body()
    finally:
        for name, _ in switches:
            monkeypatch.delenv(name)
        ctx.lib.dll.lthip_debug_reload_env()


@pytest.mark.parametrize("names", [("LTHIP_LZ4_SERIAL_DECODER",), ("LTHIP_LZ4_NO_BATCH_DECODE",), ("LTHIP_LZ4_NO_BATCH_DECODE", "LTHIP_LZ4_SERIAL_DECODER"),
                                   ("LTHIP_LZ4_PLAIN_DECODER",)], ids=["serial", "no batch", "no batch, serial", "plain"])
def test_ablation_build_ways(gpu_abl, monkeypatch, names):
    """(b) - (d): the same verdicts and bytes"""
    SMALL, LARGE, ON_PAR = groups()
    way = " ".join(f"{n}=1" for n in names)

    def body():
        check(SMALL, decode(gpu_abl, SMALL), way)
        check(LARGE, decode(gpu_abl, LARGE), f"{way}, large")

    switched(gpu_abl, monkeypatch, [(n, "1") for n in names], body)


@pytest.mark.parametrize("mib", ["1", "4096"])
def test_large_cases_origin_arena(gpu, monkeypatch, mib):
    """(e) LTHIP_ORIGIN_MIB, a switch of the product library: 1 MiB holds four units, so every block is a group of its own"""
    SMALL, LARGE, ON_PAR = groups()
    switched(gpu, monkeypatch, [("LTHIP_ORIGIN_MIB", mib)], lambda: check(LARGE, decode(gpu, LARGE), f"LTHIP_ORIGIN_MIB={mib}"))


def test_int64_instantiation(gpu):
    """(f) k_lz4_decode_lds<int64_t>: lthip_lz4_decompress_blocks selects it for the blocks of the wave-per-block decoder when one of
    them has a capacity (or a payload) of 1 GiB and more, and a payload below 64 bytes stays on that decoder whatever its capacity.
    The small cases and, last, a payload of 24 bytes with a capacity of 1 << 30.  The destination is never filled or read as a whole:
    the small windows with their guards, the first bytes of the last window and the guard behind it."""
    SMALL, LARGE, ON_PAR = groups()
    tiny = [(Z.lits(9, 1), 3, 8), (Z.lits(12, 2), None, None)]
    tiny_payload, tiny_want = np.frombuffer(Z.build(tiny), np.uint8), Z.model(tiny)
    assert len(tiny_payload) < Z.PAR_MIN_PAYLOAD
    lay = layout_of(SMALL)
    src_off = (len(lay.src) + 15) // 16 * 16 + 5
    src = np.concatenate([lay.src, W.pattern(src_off - len(lay.src) + 64)])
    src[src_off : src_off + len(tiny_payload)] = tiny_payload
    big_off = lay.dst_len + 3  # lay.dst_len: a multiple of 16 behind the last small window's guard
    HEAD = 4096                # what is looked at of the last window
    total = big_off + Z.INT64_CAP + W.GUARD
    src_offs, src_sizes = lay.src_offs + [src_off], lay.src_sizes + [len(tiny_payload)]
    dst_offs, caps = lay.dst_offs + [big_off], lay.caps + [Z.INT64_CAP]
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    first = W.pattern(big_off + HEAD + W.GUARD)
    results = []
    for fill in (first, ~first):
        d_dst[: big_off + HEAD] = torch.from_numpy(fill[: big_off + HEAD]).cuda()
        d_dst[total - W.GUARD :] = torch.from_numpy(fill[big_off + HEAD :]).cuda()
        sizes = gpu.lz4_decompress_blocks(d_src, src_offs, src_sizes, d_dst, dst_offs, caps).cpu().numpy().view(np.uint32).copy()
        low = d_dst[: big_off + HEAD].cpu().numpy()
        tail = d_dst[total - W.GUARD :].cpu().numpy()
        stray = np.flatnonzero((low[: lay.dst_len] != fill[: lay.dst_len]) & lay.outside)
        assert stray.size == 0, f"{stray.size} bytes outside every window were written, the first: {lay.blame(int(stray[0]))}"
        assert (low[lay.dst_len : big_off] == fill[lay.dst_len : big_off]).all() and (tail == fill[big_off + HEAD :]).all()
        s = int(sizes[-1])
        assert s == len(tiny_want) and low[big_off : big_off + s].tobytes() == tiny_want
        assert (low[big_off + s :] == fill[big_off + s : big_off + HEAD]).all(), "bytes behind the content of the last window were written"
        results.append([None if int(sizes[b]) == W.REFUSED else low[o : o + int(sizes[b])].tobytes() for b, o in enumerate(lay.dst_offs)])
    assert results[0] == results[1]
    check(SMALL, results[0], "int64_t instantiation")


STATS = re.compile(r"lz4 parallel decode: (\d+) blocks, (\d+) tiles \((\d+) walked again by the link pass\), (\d+) units \((\d+) given up to the origin pass\)")


def test_paths_taken(gpu_abl, monkeypatch, capfd):
    """LTHIP_LZ4_PD_STATS=1 (ablation build) reports, per call of the block-parallel path, the tiles the link pass walked again and the
    units given up to the origin pass.  One valid large case per call: the parallel-chains case has tiles neither guess entered where
    the true chain does; a case gives up exactly the units in which the census finds a match that reads below the unit's start."""
    SMALL, LARGE, ON_PAR = groups()
    valid = [e for e in LARGE if e[2] is not None]
    seen = {}

    def body():
        for e in valid:
            capfd.readouterr()
            check([e], decode(gpu_abl, [e]), "LTHIP_LZ4_PD_STATS=1")
            lines = STATS.findall(capfd.readouterr().err)
            assert len(lines) == 2 and lines[0] == lines[1], (e[0]["name"], lines)  # (two fills)
            seen[e[0]["name"], e[1]] = tuple(int(x) for x in lines[0])

    switched(gpu_abl, monkeypatch, [("LTHIP_LZ4_PD_STATS", "1")], body)
    for (name, cap), (nb, ntiles, rewalks, nunits, given_up) in seen.items():
        data = P.built(name)[0]
        c = Z.census(data)
        assert (nb, ntiles, nunits) == (1, c["ntiles"], (cap + Z.PD_UNIT - 1) // Z.PD_UNIT), name
        assert given_up == len(c["units"]), f"'{name}': {given_up} units given up, the census lists {sorted(c['units'])}"
    assert seen["parallel chains: 00 00 03 x 30000", Z.PAR_MIN_CAP][2] > 0
    assert seen["units: a source at a unit's first byte", 2 * Z.PD_UNIT][4] == 0
    assert seen["units: a source one byte below a unit's first byte", 2 * Z.PD_UNIT][4] == 1
    assert sum(1 for v in seen.values() if v[4]) >= 8
