"""Byte SOURCES for the GPU zstd encoder (k_zstd.hip: match finder, entropy stage, k_zstd_scan / k_zstd_emit), generated, not stored.
Two tables, both pure numpy:

  sources()       one source per hand-built piece of tests/zstd_encoder_units.py: the bytes its records EXECUTE to -- fresh literals
                  (skewed, noise, two symbols) and exact copies of earlier stretches at the chosen lengths and distances -- so that
                  the GPU match finder, on real bytes, lands where the unit records were put by hand.  The family (a literals,
                  b sequences, c what a unit becomes, d alignment sweep) and the claims travel with the source; what the match
                  finder makes of a source is read back with zstd_debug_units and counted from the GPU's own frames
                  (tests/test_gpu_zstd_encoder_sources.py).
  frames()        blocks of two and three 128 KiB pieces for k_zstd_scan / k_zstd_emit and the directory: every ordered pair of
                  {RLE piece, matchless raw piece, run of sub-blocks, piece that encodes to 0 after the Huffman build} -- a raw piece
                  behind a non-raw one is the one that is copied, behind raw ones only it is already in place --, last pieces of 1,
                  4095, 4096 and 4097 bytes, a piece uniform in every unit with another byte per unit, a piece uniform but for its
                  last byte, and the 1-byte piece alone."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from tests import zstd_encoder_units as E
from tests.lz4_encoder_sources import beacon_unit, differ, gram_repeats, noise, text

PIECE = 131072
U = E.U
Source = namedtuple("Source", "name family data has hasnt zero")
FAMILIES = ("a", "b", "c", "d")


@functools.lru_cache(maxsize=None)
def sources():
    out = []
    for c in E.CASES:
        raw = E.built(c["name"])[0]
        out.append(Source(c["name"], c["family"], raw, c["has"], c["hasnt"], c["zero"]))
    # The classification pass of the match finder hands a 32 KiB half-group to the lane parser only if one of its units repeats four
    # bytes inside the first 640 bytes it probes (tests/lz4_encoder_sources.py); otherwise the half is skimmed and has no sequence at
    # all.  So every source whose piece has sequences stands a second time behind a BEACON unit (B | B[:32] | noise): one more unit of
    # noise literals and one sequence in front, the units behind it as they were.
    for i, c in enumerate(E.CASES):
        raw, meta = E.built(c["name"])[:2]
        if meta[:, 0].any() and len(meta) < 32:
            out.append(Source(c["name"] + ", behind a beacon unit", c["family"], np.concatenate([beacon_unit(7000 + i), raw]), c["has"], c["hasnt"], c["zero"]))
    return out + _placed_sources()


# ---- sources placed by the match finder's own rules ---------------------------------------------------------------------------------
# Where the executed bytes of a unit case do not bring the GPU's frames to the corner, the reason is one of three rules of the match
# finder (lz4/lz4_classify.inc, lz4_lane_parse.inc, lz4_lanes_kernel.inc), and the sources below are built around them:
#   - a lane extends a match backwards no further than its own 64-byte sub-unit, and probes aligned dwords: a match that begins on a
#     sub-unit's last byte (unit offsets 255, 1023; 127 and 511 likewise) is found one byte late.  The literal counts 255 and 1023 are
#     therefore split so that the match begins at a multiple of four inside a sub-unit (128 or 252, 512 or 1020), the other literals
#     behind it, and the literals are skewed bytes mended until no four of them stand twice (one_match_unit);
#   - history enters the tables at aligned dwords only: a match is placed at a distance that is a multiple of four; and a block's last
#     match begins at least 12 bytes and ends at least 5 bytes before the block's end: a last unit keeps its literals BEHIND its match,
#     and a unit that is one match from its first byte to its last cannot be a block's last one;
#   - three to six byte values cannot fill 256 literals without a 4-byte repeat (3 values: 81 grams).  What keeps such a unit whole is
#     the classification pass: it probes the positions 0 .. 63 (a hit: the same gram 1, 2, 4 or 8 positions back), then 64, 66 .. 190
#     and 192, 195 .. against the grams probed before, and skims a group in which no probe hits.  skimmed_alphabet() lays the bytes
#     out so that none does.
def classification_sees(a):
    """whether a probe of the classification pass over a one-unit block hits (taken conservatively: a gram counts as seen when any
    position probed in an earlier batch holds it)"""
    limit = min(len(a) - 12, U - 4)
    gram = lambda p: bytes(a[p : p + 4])
    seen, pos = set(), 0
    for batch, stride in enumerate((1, 2, 3, 4)):
        ps = [pos + lane * stride for lane in range(64) if pos + lane * stride <= limit]
        if batch == 0 and any(gram(p) == gram(p - d) for p in ps for d in (1, 2, 4, 8) if p - d >= 0):
            return True
        if any(gram(p) in seen for p in ps):
            return True
        seen |= {gram(p) for p in ps}
        pos += 64 * stride
    return False


def skimmed_alphabet(bits):
    """320 bytes over the values 0 .. bits whose Huffman code is `bits` deep and in which the classification pass sees no repeat:
    0 1 2 0 1 2 .. (period 3: no gram stands 1, 2, 4 or 8 back) under the first batch, the most frequent value alone under the second,
    runs of the others under the third.  The counts are chosen so that every merge of the Huffman build takes the subtree built so far
    and one more value (6 values: 22 22 23 50 78 125): the code is a chain, `bits` deep."""
    top = bits
    a = np.zeros(320, np.uint8)
    a[:67] = np.arange(67) % 3
    a[67:192] = top
    runs = {2: [(1, 64), (0, 64)], 3: [(2, 128)], 4: [(3, 128)], 5: [(3, 50), (4, 78)]}[bits]
    at = 192
    for value, n in runs:
        a[at : at + n] = value
        at += n
    assert at == len(a) and len(set(a.tolist())) == bits + 1 and not classification_sees(a)
    return a


def skewed(n, seed):
    """n skewed bytes (Huffman pays) without a 4-byte repeat: what a parser finds in them is what was put there"""
    lit = E.Lit(seed)
    a = np.frombuffer(lit(n), np.uint8).copy()
    for _ in range(64):
        r = gram_repeats(a)
        if r.size == 0:
            return a
        a[r] = np.frombuffer(lit(r.size), np.uint8)
    raise AssertionError("the skewed bytes keep repeating")


def one_match_unit(n, front, seed):
    """three units of skewed bytes; the first begins as a beacon unit does (its bytes 64 .. 95 are its first 32), the second is `front`
    literals, the first unit's bytes front .. front + 4096 - n again (distance 4096, the match at a multiple of four and inside a
    sub-unit) and n - front literals.  No other four bytes stand twice."""
    for attempt in range(32):
        a = skewed(3 * U, seed + 1000 * attempt)
        a[64:96] = a[:32]
        differ(a, 96, a[32])
        m = U - n
        a[U + front : U + front + m] = a[front : front + m]
        differ(a, U + front - 1, a[front - 1])
        differ(a, U + front + m, a[front + m])
        r = gram_repeats(a)
        meant = ((r >= 64) & (r <= 92)) | ((r >= U + front) & (r <= U + front + m - 4))
        if meant.all():
            return a
    raise AssertionError("no seed leaves the unit its one match")


def _placed_sources():
    out = []
    for bits in (2, 3, 4, 5):
        out.append(Source(f"deepest Huffman code {bits} bits, a unit the classification pass sees no repeat in", "a", skimmed_alphabet(bits),
                          (f"huf_max_bits_{bits}", "huf_block_without_sequences", "lit_huf_tree"), (), False))
    for n, key in ((255, "lit_huf_n255"), (1023, "lit_huf_4stream_n1023")):
        for front in ((n + 1) // 2, n - 3):
            out.append(Source(f"a unit of {n} skewed literals without a repeat, {front} in front of its one match and {n - front} behind it", "a",
                              one_match_unit(n, front, 7600 + n + front), (key, "lit_huf_tree"), (), False))
    # family (c): noise, so the literals stay raw; the beacon unit has the piece parsed, N is what the probe units copy from
    for n in (31, 32):
        N, t = noise(U, 7700 + n), noise(n, 7800 + n)
        last = np.concatenate([t[:2], N[2:102], t[2:]])
        differ(last, 1, N[1])
        differ(last, 102, N[102])
        out.append(Source(f"a last unit of {n} raw literals, 2 in front of its match of 100 bytes and {n - 2} behind it", "c",
                          np.concatenate([beacon_unit(7900 + n), N, last]), (f"lit_raw_n{n}", f"lit_raw_hdr{1 if n < 32 else 2}", "last_compressed"), (), False))
    N, t = noise(U, 7750), noise(40, 7751)
    differ(t, 0, N[0])
    out.append(Source("a unit that is one match of 4096 bytes, 40 bytes of noise behind it", "c", np.concatenate([beacon_unit(7752), N, N, t]),
                      ("lit_n0", "nbseq_1"), (), False))
    return out


# ---- pieces of the multi-piece frames ----------------------------------------------------------------------------------------------------
def rle_piece(n=PIECE, byte=0x41, seed=0):
    return np.full(n, byte, np.uint8)


def raw_piece(n=PIECE, seed=1):
    """noise without a 4-byte repeat: no unit has a sequence, the piece is one Raw_Block placed by the match finder"""
    return noise(n, 9000 + seed)


def sub_piece(n=PIECE, seed=2):
    """word soup: every unit has sequences and Huffman pays: a run of sub-blocks"""
    return text(n, 9100 + seed)


def zero_piece(n=PIECE, seed=3):
    """Noise with one byte value four times as frequent as the others (1/64): neither noise test sees noise (the sampled units'
    largest count, about 256 of 16384, is above (16384 >> 7) + 4 = 132; the piece's, about 2048, above (131072 >> 7) + 4 = 1028), the
    Huffman code is built, and no unit gets smaller by it than its header costs: every unit is a Raw_Block, the total reaches
    raw_size + 3 and zb_encode_piece_sub returns 0 in phase 5.  No 4-byte repeat: nothing for the match finder."""
    rng = np.random.default_rng(9200 + seed)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    a[rng.random(n) < 3 / 256] = 0x37
    from tests.lz4_encoder_sources import gram_repeats

    for _ in range(64):
        r = gram_repeats(a)
        if r.size == 0:
            break
        a[r] = rng.integers(0, 256, r.size, dtype=np.uint8)
    assert gram_repeats(a).size == 0
    return a


def unit_uniform_piece(nunits=8):
    """every unit one repeated byte, another byte per unit: uniform units, not an RLE piece"""
    return np.repeat(np.arange(1, nunits + 1, dtype=np.uint8) * 7, E.U)


def uniform_but_last_byte(n=PIECE):
    a = np.full(n, 0x42, np.uint8)
    a[-1] = 0x43
    return a


KINDS = {"rle": rle_piece, "raw": raw_piece, "sub": sub_piece, "zero": zero_piece}
# what the directory says of a whole piece of each kind (ZDIR_RLE_PIECE, ZDIR_RAW_PIECE; None: a run of sub-block sizes)
KIND_DIRECTORY = {"rle": 0xFFFE, "raw": 0xFFFF, "sub": None, "zero": 0xFFFF}


@functools.lru_cache(maxsize=None)
def frames():
    """[(name, data, kinds per piece or None)]"""
    out = []
    for a in KINDS:
        for b in KINDS:
            out.append((f"{a} piece, then {b} piece", np.concatenate([KINDS[a](seed=1), KINDS[b](seed=2)]), (a, b)))
    for last in (1, 4095, 4096, 4097):
        out.append((f"sub, raw and a last piece of {last} bytes", np.concatenate([sub_piece(seed=4), raw_piece(seed=5), sub_piece(last, seed=6)]), None))
        out.append((f"rle, sub and a last piece of {last} noise bytes", np.concatenate([rle_piece(), sub_piece(seed=7), raw_piece(last, seed=8)]), None))
    out.append(("every unit uniform, another byte per unit", unit_uniform_piece(), None))
    out.append(("sub piece, then a piece of uniform units with different bytes", np.concatenate([sub_piece(seed=9), unit_uniform_piece(32)]), None))
    out.append(("uniform but for the last byte", uniform_but_last_byte(), None))
    out.append(("rle piece, then a piece uniform but for its last byte", np.concatenate([rle_piece(), uniform_but_last_byte()]), None))
    out.append(("one byte", np.array([0x5A], np.uint8), None))
    return out
