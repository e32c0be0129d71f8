"""Guarded layouts and case tables for the codec window tests (tests/test_gpu_codec_windows.py on the GPU, tests/test_codec_windows_cases.py
on the CPU).  The contract under test is the one longtail_hip.h states for the four block codec calls: a call writes no byte of d_dst
outside [dst_offsets[b], dst_offsets[b] + dst_caps[b]) of any block, whatever the payload holds and whatever the block's result is.

A layout places every block's source at a chosen residue mod 16 and gives it a destination window of a chosen capacity, either
"guarded" (the window starts at a chosen residue mod 16 and has at least GUARD bytes that belong to no window on either side) or
"packed" (the windows lie back to back without a gap, END_GUARD bytes at either end of the buffer).  run() makes the call twice, on a
destination filled with a position-dependent pattern and on one filled with its complement, and reports every byte outside the union
of the windows that no longer holds its fill: a stray byte that happens to equal one fill cannot equal the other.

Expected bytes and verdicts come from the oracle, the reference and the source data only; nothing here loads the library under test."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

GUARD = 96       # bytes beside every window in guarded mode
END_GUARD = 256  # bytes at either end of the destination in packed mode
REFUSED = 0xFFFFFFFF

# ---- layouts ---------------------------------------------------------------------------------------------------------------------


def pattern(n: int) -> np.ndarray:
    """The fill: a byte that depends on its position (a multiplicative hash of it), so that a block of bytes copied to the wrong place,
    or a constant, shows up.  run() also uses its complement."""
    i = np.arange(n, dtype=np.uint32)
    return ((i * np.uint32(2654435761)) >> np.uint32(24)).astype(np.uint8)


@dataclass
class Layout:
    mode: str
    specs: list       # (source residue, destination residue, capacity) per block, as asked for
    src: np.ndarray   # the source buffer: the blocks at their residues, the fill pattern in between
    src_offs: list
    src_sizes: list
    dst_len: int
    dst_offs: list
    caps: list
    outside: np.ndarray  # bool per destination byte: True where it belongs to no window

    def describe(self, b: int) -> str:
        s, d, cap = self.specs[b]
        return (f"block {b} (source residue, destination residue, length, capacity) = ({s}, {self.dst_offs[b] % 16}, "
                f"{self.src_sizes[b]}, {cap}), {self.mode}")

    def blame(self, pos: int) -> str:
        """The window nearest to a destination position outside all windows, and where the position lies from it."""
        starts = np.asarray(self.dst_offs, np.int64)
        ends = starts + np.asarray(self.caps, np.int64)
        dist = np.where(pos < starts, starts - pos, pos - ends + 1)
        b = int(np.argmin(dist))
        where = f"{int(starts[b]) - pos} bytes in front of" if pos < starts[b] else f"{pos - int(ends[b]) + 1} bytes past the end of"
        return f"destination byte {pos}, {where} the window of {self.describe(b)}"


def build_layout(blocks, specs, mode: str, same_source: "Layout | None" = None) -> Layout:
    """same_source: a layout of the same blocks at the same source residues (other capacities), whose source buffer is taken over"""
    assert mode in ("guarded", "packed") and len(blocks) == len(specs)
    if same_source is not None:
        src, src_offs = same_source.src, same_source.src_offs
        assert [o % 16 for o in src_offs] == [s for s, _, _ in specs] and same_source.src_sizes == [len(b) for b in blocks]
    else:
        src_offs, pos = [], 0
        for blk, (s, _, _) in zip(blocks, specs):
            pos = (pos + 15) // 16 * 16 + s
            src_offs.append(pos)
            pos += len(blk)
        src = pattern((pos + 15) // 16 * 16 + 64)
        for o, blk in zip(src_offs, blocks):
            src[o : o + len(blk)] = blk
    dst_offs = []
    if mode == "guarded":
        pos = 0
        for _, d, cap in specs:
            pos = (pos + 15) // 16 * 16 + GUARD + d  # (GUARD is a multiple of 16: the window starts at residue d)
            dst_offs.append(pos)
            pos += cap
        dst_len = (pos + GUARD + 15) // 16 * 16
    else:
        pos = END_GUARD
        for _, _, cap in specs:
            dst_offs.append(pos)
            pos += cap
        dst_len = (pos + END_GUARD + 15) // 16 * 16
    outside = np.ones(dst_len, bool)
    for o, (_, _, cap) in zip(dst_offs, specs):
        outside[o : o + cap] = False
    return Layout(mode, list(specs), src, src_offs, [len(b) for b in blocks], dst_len, dst_offs, [c for _, _, c in specs], outside)


@dataclass
class Result:
    sizes: np.ndarray  # u32 per block, as the call returned them
    windows: list      # every block's whole window (capacity bytes) after the call
    stray: np.ndarray  # positions outside all windows that no longer hold the fill


def run(lay: Layout, call):
    """call(d_src, src_offs, src_sizes, d_dst, dst_offs, caps) -> device u32 sizes.  -> [Result on the pattern, Result on its complement]"""
    import torch

    d_src = torch.from_numpy(lay.src).cuda()
    first = pattern(lay.dst_len)
    out = []
    for fill in (first, ~first):
        d_dst = torch.from_numpy(fill).cuda()
        assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
        sizes = call(d_src, lay.src_offs, lay.src_sizes, d_dst, lay.dst_offs, lay.caps).cpu().numpy().view(np.uint32).copy()
        got = d_dst.cpu().numpy()
        stray = np.flatnonzero((got != fill) & lay.outside)
        out.append(Result(sizes, [got[o : o + c] for o, c in zip(lay.dst_offs, lay.caps)], stray))
    return out


def check_guards(lay: Layout, results) -> None:
    for which, r in zip(("pattern", "complement"), results):
        assert r.stray.size == 0, (f"{r.stray.size} bytes outside every window were written ({which} fill), the first: "
                                   f"{lay.blame(int(r.stray[0]))}")


# ---- LZ4 decode: valid payloads and payloads that want more room ------------------------------------------------------------------

# around DEC_FLUSH, DEC_RING, the direct long-literal path (3 * DEC_RING), PD_UNIT, and the block-parallel path (2 * PD_UNIT and up)
LZ4_DEC_SIZES = [0, 1, 15, 16, 17, 2047, 2048, 2049, 8191, 8192, 8193, 24575, 24576, 24577, 65535, 65536, 65537, 131071, 131072, 131073,
                 200000]
LZ4_DEC_CONTENTS = ("noise", "zeros", "synth1")
LZ4_DEC_SRC_RES = (0, 1, 2, 3, 5, 15)
LZ4_OVERSHOOTS = (1, 2, 15, 16, 17, 63, 64, 65, 2048, 70000)
LZ4_TAILS = ("noise", "zeros", "zeros+5")


def lz4_raw(oracle, n: int, content: str) -> np.ndarray:
    if content == "zeros":
        return np.zeros(n, np.uint8)
    return oracle.synth(n, 1000 + n, 0 if content == "noise" else 1)


def lz4_literal_run_size(n: int) -> int:
    """the payload of n bytes without a match: a token, the length bytes of n >= 15, the bytes"""
    return 1 + (0 if n < 15 else (n - 15) // 255 + 1) + n


def lz4_valid_payloads(oracle, content: str):
    """[(raw, payload of the oracle's LZ4_compress_fast restatement)] per size of LZ4_DEC_SIZES"""
    raws = [lz4_raw(oracle, n, content) for n in LZ4_DEC_SIZES]
    return [(r, oracle.lz4_compress(r)) for r in raws]


def lz4_valid_cases(oracle, content: str):
    """Every size x every destination residue x the source residues: (raw, payload, source residue, destination residue)."""
    return [(r, p, s, d) for r, p in lz4_valid_payloads(oracle, content) for d in range(16) for s in LZ4_DEC_SRC_RES]


def lz4_overshoot_cases(oracle):
    """A raw of n + k bytes, compressed, offered with a capacity of n: dict(payload, cap, k, tail, sres, dres).  The raw is synth kind 1 with
    its last k + 40 bytes replaced by noise (the final literal run overshoots), zeros (the last match does) or zeros and 5 noise bytes."""
    cases = []
    for n in LZ4_DEC_SIZES:
        if n < 16:
            continue
        for k in LZ4_OVERSHOOTS:
            for tail in LZ4_TAILS:
                raw = oracle.synth(n + k, 2000 + n + k, 1)
                t = min(n + k, k + 40)
                raw[n + k - t :] = oracle.synth(t, 3000 + n + k, 0) if tail == "noise" else 0
                if tail == "zeros+5":
                    raw[n + k - 5 :] = oracle.synth(5, 4000 + n + k, 0)
                i = len(cases)
                cases.append(dict(payload=oracle.lz4_compress(raw), cap=n, k=k, tail=tail, sres=LZ4_DEC_SRC_RES[i % 6], dres=(1 + 7 * i) % 16))
    return cases


# ---- LZ4 decode: damaged payloads -------------------------------------------------------------------------------------------------
# The mutation generators of test_lz4_gpu_decoder_differential_fuzz and test_lz4_block_parallel_decoder_differential_fuzz
# (tests/test_gpu_codecs.py), statement for statement and with their seeds, so that the same damaged payloads meet guarded windows.


def lz4_fuzz_cases(oracle):
    """[(payload, capacity)] of test_lz4_gpu_decoder_differential_fuzz"""
    rng = np.random.default_rng(77)
    raws = [oracle.synth(n, 300 + n, k) for k, n in ((1, 70000), (1, 9000), (2, 5000), (0, 3000), (11, 40000), (12, 20000))]
    raws.append(np.frombuffer(b"abcdefgh" * 3000 + b"x" * 70000 + bytes(range(256)) * 40, np.uint8).copy())
    far = rng.integers(0, 256, 30000, dtype=np.uint8)
    raws.append(np.concatenate([far, rng.integers(0, 256, 20000, dtype=np.uint8), far]))
    cases = []
    for raw in raws:
        comp = oracle.lz4_compress(raw)
        cases.append((comp, len(raw)))
        for _ in range(24):
            c = comp.copy()
            kind = rng.integers(0, 5)
            if kind == 0 and len(c) > 2:
                c = c[: rng.integers(1, len(c))]
            elif kind == 1:
                for _ in range(rng.integers(1, 4)):
                    c[rng.integers(0, len(c))] ^= 1 << rng.integers(0, 8)
            elif kind == 2:
                c[rng.integers(0, len(c)) :] = 0
            elif kind == 3:
                c[rng.integers(0, len(c))] = 255
            cap = len(raw) if kind != 4 else max(0, len(raw) + int(rng.integers(-20, 20)))
            cases.append((c, cap))
    return cases


def lz4_pd_fuzz_raws(oracle):
    raws = [oracle.synth(n, 40 + k, k) for k, n in ((1, 400000), (11, 262144), (12, 150000), (0, 140000))]
    raws.append(np.concatenate([oracle.synth(100000, 3, 1), np.zeros(300000, np.uint8), oracle.synth(50000, 4, 1)]))
    return raws


def lz4_pd_fuzz_cases(oracle, raws, own_payloads):
    """[(payload, capacity)] of test_lz4_block_parallel_decoder_differential_fuzz; own_payloads: the HIP encoder's payloads of `raws`"""
    rng = np.random.default_rng(4711)
    cases = []
    for raw, own in zip(raws, own_payloads):
        for comp in (oracle.lz4_compress(raw), own):
            cases.append((comp, len(raw)))
            for _ in range(16):
                c = comp.copy()
                kind = rng.integers(0, 6)
                if kind == 0:
                    c = c[: rng.integers(1, len(c))]
                elif kind == 1:
                    for _ in range(rng.integers(1, 4)):
                        c[rng.integers(0, len(c))] ^= 1 << rng.integers(0, 8)
                elif kind == 2:
                    c[rng.integers(0, len(c)) :] = 0
                elif kind == 3:
                    c[rng.integers(0, len(c))] = 255
                elif kind == 4:
                    a = rng.integers(0, len(c) - 2)
                    c[a : a + 2] = 0
                cap = len(raw) if kind != 5 else max(131072, len(raw) + int(rng.integers(-70000, 70000)))
                cases.append((c, cap))
    return cases


# ---- zstd ---------------------------------------------------------------------------------------------------------------------------

ZSTD_DEC_SIZES = [0, 1, 100, 4095, 4096, 4097, 131071, 131072, 131073, 400000]
ZSTD_KINDS = (0, 1, 12, "zeros")
ZSTD_CHAIN_SIZE = 9 * 131072 + 77  # quality 2 runs eight pieces in a row as a chain (every eighth piece starts a new one)
ZSTD_DEC_DST_RES = (0, 1, 7, 8, 15)
ZSTD_DEC_SRC_RES = (0, 1, 3)
ZSTD_SHORT_BY = (1, 16, 4096, 131072)


def zstd_raw(oracle, n: int, kind) -> np.ndarray:
    return np.zeros(n, np.uint8) if kind == "zeros" else oracle.synth(n, 500 + n, kind)


def zstd_raws(oracle):
    return [zstd_raw(oracle, n, k) for k in ZSTD_KINDS for n in ZSTD_DEC_SIZES]


def zstd_damaged_frames(oracle, ref):
    """[(frame, capacity)] of test_zstd_decoder_agrees_with_host_model_and_reference_on_damaged_frames (tests/test_gpu_codecs.py),
    statement for statement and with its seed."""
    rng = np.random.default_rng(4)
    cases = []
    for kind, n in ((1, 200000), (11, 30000), (12, 100000), (13, 60000), (1, 3000)):
        b = oracle.synth(n, 31 + n, kind)
        for w in (0, 2):
            c = ref.compress(1, ref.dll.refh_zstd_type(w), b)
            for _ in range(60):
                x = c.copy()
                if rng.integers(0, 4) == 0:
                    x = x[: rng.integers(0, len(x) + 1)].copy()
                else:
                    for _ in range(int(rng.integers(1, 4))):
                        x[rng.integers(0, len(x))] ^= np.uint8(1 << rng.integers(0, 8))
                cases.append((x, n if rng.integers(0, 3) else int(rng.integers(0, n + 1))))
    return cases


def zstd_trailer_size(n: int) -> int:
    """the directory trailer of a frame of n > 0 content bytes: a skippable-frame header, the tag, one u16 per 4 KiB unit"""
    return 12 + 2 * ((n + 4095) // 4096)


# ---- the encoders -------------------------------------------------------------------------------------------------------------------

ENC_SRC_RES = (0, 1, 3, 15)
LZ4_ENC_SIZES = [0, 1, 12, 13, 4095, 4096, 4097, 65535, 65536, 65537, 200000]
LZ4_ENC_KINDS = (0, 1, 2)
ZSTD_ENC_SIZES = [0, 1, 4096, 131072, 131073, 400000]
ZSTD_ENC_KINDS = (0, 1, 2, "zeros")


def lz4_bound(n: int) -> int:
    return n + n // 255 + 16  # LZ4_COMPRESSBOUND (tests/test_abi.py holds lthip_lz4_bound to it)


def zstd_bound(n: int) -> int:
    return n + (n >> 8) + (((128 << 10) - n) >> 11 if n < (128 << 10) else 0)  # ZSTD_COMPRESSBOUND (tests/test_abi.py, likewise)


def enc_cases(oracle, sizes, kinds):
    """Every size x kind x source residue x destination residue: (raw, source residue, destination residue, kind)."""
    raws = [(zstd_raw(oracle, n, k), k) for k in kinds for n in sizes]
    return [(r, s, d, k) for r, k in raws for s in ENC_SRC_RES for d in range(16)]


def lz4_noise_cut_caps(n: int):
    """capacities that end inside a 4 KiB unit of the one literal run a noise block becomes: 1 + length bytes + j * 4096 + r"""
    head = lz4_literal_run_size(n) - n
    return [head + j * 4096 + r for j in (0, 1, 15) for r in (0, 1, 4095)]
