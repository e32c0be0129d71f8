"""The hand-built zstd frames (tests/zstd_format.py writes them) and the feature list they and the reference encoder's frames must
cover.  A case is (name, spec, features, verdict, path):
  features  census keys the frame was built for (tests/test_zstd_format_cases.py asserts the census finds each of them)
  verdict   "valid" | "invalid" (a near miss: one step outside the format, rejected by the reference and by every decoder here) |
            "stricter" (outside the format as RFC 8878 states it, yet the reference decodes it: the decoders here reject it, which the
            one-sided rule allows) | "checksum" (wrong content checksum: the one documented case the decoders accept and the
            reference rejects, zstd_decode_core.h: the checksum is skipped)
  path      what k_zstd_decode.hip does with a VALID frame, from its code:
            "parallel"    listed by k_zstd_split, decoded block-parallel
            "unlisted"    never listed (z_split_foreign returns false): no content size, zero content, more than one frame in the
                          payload, more than ZF_SLOTS blocks per 128 KiB of capacity -- the serial decoder from the start
            "handed_back" listed, then given back through d_retry to k_zstd_decode_retry: an Offset_Value of 2^24 or more, a
                          record arena too small for one sequence per three bytes, a literal stream of no symbols (the fourth
                          stream of six literals: k_zstd_blk_entropy takes a stream without symbols for damage)
  large     the two frames of 8 MiB and more (left out of the replicated calls)
Nothing here loads the library under test."""
from __future__ import annotations

from functools import lru_cache

from tests.zstd_format import (LL, LL_BASE, LL_BITS, ML, ML_BASE, ML_BITS, OF, build, compressed, frame, lit_huf, lit_raw, lit_rle,
                               lit_treeless, off, raw, rle, skippable)


def noise(n: int, seed: int, alphabet: int = 256, skew: int = 1) -> bytes:
    """n bytes of a 64-bit LCG, values below `alphabet`; skew > 1 makes small values more frequent (a tree with several depths)"""
    x, out = seed * 2 + 1, bytearray(n)
    for i in range(n):
        x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
        v = x >> 33
        for _ in range(skew - 1):
            x = (x * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
            v = min(v % alphabet, (x >> 33) % alphabet)
        out[i] = v % alphabet
    return bytes(out)


# frames with small compressed blocks carry a Window_Descriptor: a single-segment frame's window is its content, and a block may not
# be larger than the window (3.1.1.2: Block_Maximum_Size) -- a few literals cost more bytes than they regenerate
WIN = dict(single=False, window_log=17, fcs=4)
BIG = dict(single=False, window_log=25, fcs=4)
CASES = []


def case(name, spec, features=(), verdict="valid", path="parallel", large=False, cap_extra=0):
    CASES.append(dict(name=name, spec=spec, features=tuple(features), verdict=verdict, path=path if verdict == "valid" else None,
                      large=large, cap_extra=cap_extra))


def _simple(n=3, seed=1):
    """a compressed block of raw literals and three sequences (a new offset, a repeated one with and without literals)"""
    return compressed(lit_raw(noise(8 + n, seed)), [(4, 5, off(2)), (2, 3, 1), (0, 4, 1)])


# ---- frame header -----------------------------------------------------------------------------------------------------------------
case("fcs 1 byte, content 255", lambda: frame([raw(noise(255, 1))]), ["single_segment", "fcs_1", "fcs_1_content_255", "last_raw"])
case("fcs 2 bytes, content 256", lambda: frame([raw(noise(256, 2))]), ["fcs_2", "fcs_2_content_256"])
case("fcs 2 bytes, content 65791", lambda: frame([raw(noise(65791, 3))]), ["fcs_2", "fcs_2_content_65791"])
case("fcs 4 bytes", lambda: frame([raw(noise(100, 4)), _simple()], fcs=4), ["fcs_4", "single_segment", "last_compressed"])
case("fcs 8 bytes", lambda: frame([raw(noise(100, 5)), rle(9, 50)], fcs=8), ["fcs_8", "last_rle"])
case("window descriptor and fcs", lambda: frame([_simple()], **WIN), ["window_with_fcs"])
case("window descriptor, no fcs", lambda: frame([_simple()], single=False, window_log=17, fcs=0), ["window_without_fcs", "fcs_0"],
     path="unlisted")
case("content checksum", lambda: frame([raw(noise(300, 6)), _simple()], checksum=True), ["checksum"])
case("wrong content checksum", lambda: frame([raw(noise(300, 6)), _simple()], checksum=True, checksum_xor=1), verdict="checksum")
case("reserved header bit", lambda: frame([raw(noise(40, 7))], reserved=True), verdict="invalid")
case("dictionary id", lambda: frame([raw(noise(40, 8))], dict_id=5), verdict="invalid")
case("content size one too large", lambda: frame([raw(noise(40, 9)), _simple()], fcs=4, fcs_delta=1), verdict="invalid", cap_extra=2)
case("content size one too small", lambda: frame([raw(noise(40, 10)), _simple()], fcs=4, fcs_delta=-1), verdict="invalid", cap_extra=2)
case("zero content", lambda: frame([raw(b"")]), ["content_0", "raw_block_empty_last"], path="unlisted")
case("two frames", lambda: [frame([raw(noise(70, 11))]), frame([_simple()], **WIN)], ["concatenated"], path="unlisted")
case("skippable frame first", lambda: [skippable(), frame([raw(noise(70, 12))])], ["skippable_first"], path="unlisted")
case("skippable frame between", lambda: [frame([raw(noise(70, 13))]), skippable(b"", 3), frame([rle(1, 9)])],
     ["skippable_after_frame", "concatenated"], path="unlisted")
case("skippable frame last", lambda: [frame([raw(noise(70, 14))]), skippable(b"\x01\x02\x03", 15)], ["skippable_last"], path="unlisted")

# ---- blocks -------------------------------------------------------------------------------------------------------------------------
case("empty raw block in mid-frame", lambda: frame([raw(b"ab"), raw(b""), rle(3, 5)]), ["raw_block_empty_mid", "block_rle", "block_raw"])
case("rle block of 131072", lambda: frame([rle(7, 131072)]), ["rle_block_131072"])
case("compressed block regenerates 131072",
     lambda: frame([compressed(lit_rle(5, 10), [(10, 131062, off(1))])], **WIN), ["compressed_block_131072", "offset_1_long_match"])
case("compressed block regenerates 131073", lambda: frame([compressed(lit_rle(5, 10), [(10, 131063, off(1))])], **WIN), verdict="stricter")
case("block type 3", lambda: frame([raw(noise(30, 15))], block_type3=0), verdict="invalid")
case("nine blocks in 90 bytes", lambda: frame([raw(noise(10, 20 + i)) for i in range(9)]), ["block_raw"], path="unlisted")
case("compressed block larger than a single-segment frame's window",
     lambda: frame([compressed(lit_huf(bytes([1, 2, 1, 1, 3, 1]), streams=1), [])]), verdict="invalid")

# ---- literals -----------------------------------------------------------------------------------------------------------------------
case("raw literals at the header-size edges", lambda: frame([compressed(lit_raw(noise(n, 30 + n)), []) for n in (31, 32, 4095, 4096)], **WIN),
     ["lit_raw_n31", "lit_raw_n32", "lit_raw_n4095", "lit_raw_n4096", "lit_raw_hdr1", "lit_raw_hdr2", "lit_raw_hdr3", "nbseq_0"])
case("rle literals at the header-size edges", lambda: frame([compressed(lit_rle(n & 255, n), []) for n in (31, 32, 4095, 4096)], **WIN),
     ["lit_rle_n31", "lit_rle_n32", "lit_rle_n4095", "lit_rle_n4096", "lit_rle_hdr1", "lit_rle_hdr2", "lit_rle_hdr3"])
case("one stream of 1023 literals", lambda: frame([compressed(lit_huf(noise(1023, 40, 9, 2), streams=1), [])], **WIN),
     ["lit_huf_1stream_n1023", "huf_stream_long", "huf_direct_even"])
case("four streams of 1024 literals", lambda: frame([compressed(lit_huf(noise(1024, 41, 6, 2), streams=4), [])], **WIN),
     ["lit_huf_4stream_n1024", "lit_huf_hdr4", "huf_direct_odd"])
case("four streams of 16383 literals", lambda: frame([compressed(lit_huf(noise(16383, 42, 20, 2), streams=4), [])], **WIN),
     ["lit_huf_4stream_n16383", "lit_huf_hdr4"])
case("four streams of 16384 literals", lambda: frame([compressed(lit_huf(noise(16384, 43, 33, 3), streams=4), [(7, 9, off(5))])], **WIN),
     ["lit_huf_4stream_n16384", "lit_huf_hdr5"])
SIX = "four streams of 6 literals"
case(SIX, lambda: frame([compressed(lit_huf(bytes([1, 2, 1, 1, 3, 1]), streams=4), [])], **WIN),
     ["lit_huf_4stream_n6", "lit_huf_last_stream_empty", "huf_stream_short"], path="handed_back")
case("four streams of 5 literals", lambda: frame([compressed(lit_huf(bytes([1, 2, 1, 1, 3]), streams=4), [])], **WIN), verdict="invalid")
case("tree of two symbols", lambda: frame([compressed(lit_huf(noise(50, 44, 2), streams=1, weights=[1, 1]), [(3, 4, off(2))])], **WIN),
     ["huf_two_symbols", "huf_direct_odd", "huf_max_bits_1", "huf_stream_short"])
case("tree with codes of 11 bits",
     lambda: frame([compressed(lit_huf(bytes(range(12)) * 3 + noise(400, 45, 3), streams=1, weights=[11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]),
                               [(30, 8, off(12))])], **WIN), ["huf_max_bits_11", "huf_direct_odd"])
case("treeless directly after its tree",
     lambda: frame([compressed(lit_huf(noise(200, 46, 5, 2), streams=1), [(9, 4, off(3))]),
                    compressed(lit_treeless(noise(300, 47, 5, 2), streams=4), [(5, 6, off(100))])], **WIN), ["treeless_directly_after_tree", "lit_treeless"])
case("treeless after raw literals and raw / rle blocks",
     lambda: frame([compressed(lit_huf(noise(200, 48, 7, 2), streams=1), []), compressed(lit_raw(noise(20, 49)), [(9, 4, off(3))]), raw(noise(33, 50)),
                    rle(4, 17), compressed(lit_treeless(noise(90, 51, 7, 2), streams=1), [(5, 6, off(100))])], **WIN),
     ["treeless_after_raw_literals", "treeless_after_raw_rle_block"])
case("treeless in the first block", lambda: frame([raw(noise(9, 52)), compressed(lit_treeless(bytes([0, 1, 1, 0, 1] * 4), force=True), [])], **WIN),
     verdict="invalid")
case("literal stream ends in a zero byte", lambda: frame([compressed(lit_huf(noise(200, 53, 5, 2), streams=1, zero_last_byte=True), [])], **WIN),
     verdict="invalid")
case("literal stream with a bit left over", lambda: frame([compressed(lit_huf(noise(200, 54, 5, 2), streams=1, extra_bit=True), [])], **WIN),
     verdict="invalid")
case("fourth literal stream with a bit left over", lambda: frame([compressed(lit_huf(noise(2000, 55, 5, 2), streams=4, extra_bit=True), [])], **WIN),
     verdict="stricter")


# ---- sequence section ---------------------------------------------------------------------------------------------------------------
def _counted(n):
    """n sequences of three bytes each at a new offset 1, one literal in front"""
    return frame([compressed(lit_raw(b"\x42"), [(1, 3, off(1))] + [(0, 3, off(1))] * (n - 1))], **WIN)


for _n, _key in ((1, "nbseq_1"), (127, "nbseq_127"), (128, "nbseq_128"), (0x7EFF, "nbseq_32511"), (0x7F00, "nbseq_ge_0x7F00")):
    case(f"{_n} sequences", (lambda n=_n: _counted(n)), [_key, f"nbseq_{1 if _n < 128 else 2 if _n < 0x7F00 else 3}byte"])
case("127 sequences, the count in two bytes", lambda: frame([compressed(lit_raw(b"\x42"), [(1, 3, off(1))] + [(0, 3, off(1))] * 126, count_bytes=2)], **WIN),
     ["nbseq_127", "nbseq_2byte"])

_VARIED = [(4, 5, off(2)), (2, 3, 1), (0, 4, 1), (1, 40, off(9)), (17, 3, off(30)), (0, 70, off(1)), (3, 9, 2), (2, 4, 3)]
_SAME = [(1, 4, off(1))] * 5


def _lits(seqs, seed, extra=3):
    return lit_raw(noise(sum(s[0] for s in seqs) + extra, seed))


case("every table predefined", lambda: frame([compressed(_lits(_VARIED, 60), _VARIED)], **WIN), ["ll_predefined", "of_predefined", "ml_predefined"])
case("every table rle", lambda: frame([compressed(_lits(_SAME, 61), _SAME, modes=("rle",) * 3)], **WIN), ["ll_rle", "of_rle", "ml_rle"])
case("every table fse", lambda: frame([compressed(_lits(_VARIED, 62), _VARIED, modes=("fse",) * 3)], **WIN), ["ll_fse", "of_fse", "ml_fse"])
case("mixed table modes", lambda: frame([compressed(_lits(_SAME, 63), _SAME, modes=("fse", "rle", "predefined")),
                                         compressed(_lits(_SAME, 64), _SAME, modes=("rle", "predefined", "fse"))], **WIN), ["ll_fse", "of_rle", "ml_fse"])
case("repeat after fse", lambda: frame([compressed(_lits(_VARIED, 65), _VARIED, modes=("fse",) * 3),
                                        compressed(_lits(_VARIED, 66), _VARIED, modes=("repeat",) * 3)], **WIN),
     ["ll_repeat", "of_repeat", "ml_repeat", "repeat_after_fse", "repeat_directly"])
case("repeat after predefined", lambda: frame([compressed(_lits(_VARIED, 67), _VARIED),
                                               compressed(_lits(_VARIED, 68), _VARIED, modes=("repeat",) * 3)], **WIN), ["repeat_after_predefined"])
case("repeat after rle", lambda: frame([compressed(_lits(_SAME, 69), _SAME, modes=("rle",) * 3),
                                        compressed(_lits(_SAME, 70), _SAME, modes=("repeat",) * 3)], **WIN), ["repeat_after_rle"])
case("repeat across a block without sequences",
     lambda: frame([compressed(_lits(_VARIED, 71), _VARIED, modes=("fse",) * 3), compressed(lit_raw(noise(12, 72)), []),
                    compressed(_lits(_VARIED, 73), _VARIED, modes=("repeat",) * 3)], **WIN), ["repeat_across_zero_seq_block"])
case("repeat across raw and rle blocks",
     lambda: frame([compressed(_lits(_VARIED, 74), _VARIED, modes=("fse",) * 3), raw(noise(12, 75)), rle(8, 21),
                    compressed(_lits(_VARIED, 76), _VARIED, modes=("repeat",) * 3)], **WIN), ["repeat_across_raw_rle_block"])
case("repeat in the first block", lambda: frame([raw(noise(20, 77)), compressed(_lits(_VARIED, 78), _VARIED, modes=("repeat", "predefined", "predefined"))], **WIN),
     verdict="invalid")
for _t, _name in ((LL, "literal-length"), (OF, "offset"), (ML, "match-length")):
    case(f"{_name} table log above its maximum", (lambda t=_t: frame([compressed(_lits(_VARIED, 79), _VARIED, modes=("fse",) * 3, log_over=t)], **WIN)),
         verdict="invalid")
case("normalised count one short of its table", lambda: frame([compressed(_lits(_VARIED, 80), _VARIED, modes=("fse",) * 3, ncount_short=ML)], **WIN),
     verdict="invalid")
case("sequence bit-stream with a bit left over", lambda: frame([compressed(_lits(_VARIED, 81), _VARIED, extra_bit=True)], **WIN), verdict="invalid")
case("sequence bit-stream ends in a zero byte", lambda: frame([compressed(_lits(_VARIED, 82), _VARIED, zero_last_byte=True)], **WIN), verdict="invalid")
case("reserved mode bits", lambda: frame([compressed(_lits(_VARIED, 83), _VARIED, reserved=1)], **WIN), verdict="invalid")


EIGHT = "eight compressed blocks"  # (the most a frame of up to 128 KiB may have and stay block-parallel: ZF_SLOTS)
case(EIGHT, lambda: frame([compressed(_lits(_VARIED, 84 + i), _VARIED, modes=(("fse",) * 3, ("repeat",) * 3, ("predefined", "fse", "fse"),
                                                                                ("repeat", "fse", "repeat"))[i % 4]) for i in range(8)], **WIN),
     ["block_compressed", "repeat_after_fse"])


# ---- codes --------------------------------------------------------------------------------------------------------------------------
def _top(base, bits, c, limit):
    """a value of code c: its largest below `limit` codes (all extra bits set), its baseline above"""
    return base[c] + ((1 << bits[c]) - 1 if c < limit else 0)


def _all_length_codes():
    a = [(_top(LL_BASE, LL_BITS, c, 28) if c < 34 else 0, _top(ML_BASE, ML_BITS, c, 44), off(1 + c)) for c in range(34)]
    a += [(c % 3, _top(ML_BASE, ML_BITS, c, 44), off(c)) for c in range(34, 51)]
    a[0] = (1, a[0][1], off(1))  # (something must be there to copy)
    blocks = [a, [(LL_BASE[34] + 77, ML_BASE[51] + 5, off(40000))], [(LL_BASE[35] + 1, 3, off(3))], [(2, ML_BASE[52] + 60000, off(2))]]
    return frame([compressed(_lits(s, 90 + i), s) for i, s in enumerate(blocks)], **BIG)


case("every literal-length and match-length code", _all_length_codes,
     [f"ll_code_{c}" for c in range(36)] + [f"ml_code_{c}" for c in range(53)])

# tables of accuracy logs 9 / 8 / 9 in which every code but the first has one cell: a state of such a code takes all the table's bits
_WIDE = ([512 - 35] + [1] * 35, [256 - 24] + [1] * 24, [512 - 52] + [1] * 52)


def _far_blocks(n):
    """128 KiB of noise, then n - 1 RLE blocks of 128 KiB, every one another byte"""
    return [raw(noise(131072, 99))] + [rle((i * 37 + 11) & 255, 131072) for i in range(1, n)]


def _offset_codes():
    """65 blocks of 128 KiB in front, so that offsets of every code up to 23 exist: one sequence per code, then a block whose first
    sequence has 54 extra bits and is followed by 26 state bits (more than one 64-bit view holds)"""
    seqs = [(1, 3, off(1))] + [(1 + c % 2, 3 + c, (1 << c) + (1 << c) // 70 + (c & 1)) for c in range(2, 24)] + [(1, 3, 1), (0, 3, 1), (1, 3, 2)]
    wide = [(LL_BASE[34] + 5, ML_BASE[52] + 7, (1 << 23) + 12345), (0, 3, off(1)), (0, 5, off(70000))]
    return frame(_far_blocks(65) + [compressed(_lits(seqs, 100), seqs), compressed(_lits(wide, 101), wide, modes=("fse",) * 3, norms=_WIDE, logs=(9, 8, 9))],
                 **BIG)


case("every offset code up to 23, and a sequence of 80 bits", _offset_codes,
     [f"of_code_{c}" for c in range(24)] + ["seq_bits_above_64", "of_codes_above_23_unused", "rle_block_131072", "match_reads_raw_block",
                                            "match_reads_rle_block"], large=True)


def _offset_codes_mid():
    """the same with three blocks of 128 KiB in front: offset codes up to 18, and a sequence of 49 extra and 26 state bits -- small
    enough for the replicated calls, so that every sequence walker of the product build fetches its second bit window"""
    seqs = [(1, 3, off(1))] + [(1 + c % 2, 3 + c, (1 << c) + (1 << c) // 70 + (c & 1)) for c in range(2, 19)]
    wide = [(LL_BASE[34] + 5, ML_BASE[52] + 7, (1 << 18) + 999), (0, 3, off(1)), (0, 5, off(70000))]
    return frame(_far_blocks(3) + [compressed(_lits(seqs, 105), seqs), compressed(_lits(wide, 106), wide, modes=("fse",) * 3, norms=_WIDE, logs=(9, 8, 9))],
                 **BIG)


WIDE_MID = "offset codes up to 18, and a sequence of 75 bits"
case(WIDE_MID, _offset_codes_mid, [f"of_code_{c}" for c in range(2, 19)] + ["seq_bits_above_64", "of_codes_above_23_unused", "match_reads_raw_block",
                                                                            "match_reads_rle_block"])
case("offset value of 2^24 and more", lambda: frame(_far_blocks(129) + [compressed(lit_raw(noise(9, 102)), [(4, 300, (1 << 24) + 777), (2, 9, 1)])], **BIG),
     ["offset_value_ge_2p24", "of_code_24"], path="handed_back", large=True)
case("offset table that holds codes 24 to 28, unused",
     lambda: frame([compressed(_lits(_VARIED, 104), _VARIED, modes=("predefined", "fse", "predefined"), norms=(None, [5] * 8 + [1] * 8 + [0] * 8 + [-1] * 5 + [11], None),
                               logs=(None, 6, None))], **WIN), ["of_codes_above_23_unused", "of_table_holds_codes_above_23"])

# ---- offsets ------------------------------------------------------------------------------------------------------------------------
_REPS = [(4, 4, off(7)), (2, 4, off(5)), (3, 4, off(3)), (1, 3, 1), (1, 3, 2), (1, 3, 3), (0, 3, 1), (0, 3, 2), (0, 3, 3), (2, 5, off(9)), (0, 4, 3)]
case("every repeat-offset form", lambda: frame([raw(noise(16, 110)), compressed(_lits(_REPS, 111), _REPS)], **WIN),
     [f"offset_value_{v}_{k}" for v in (1, 2, 3) for k in ("ll", "ll0")] + ["repeat1_minus_one"])
case("repeat 1 minus one is zero", lambda: frame([raw(noise(16, 112)), compressed(lit_raw(noise(5, 113)), [(2, 3, off(1)), (0, 3, 3)])], **WIN),
     verdict="invalid")
case("initial offset history in the first block", lambda: frame([compressed(lit_raw(noise(12, 114)), [(8, 4, 3), (1, 3, 3), (1, 3, 3)])], **WIN),
     ["initial_history_8_used", "initial_history_4_used", "initial_history_1_used", "initial_history_in_first_block", "offset_eq_position"])
case("initial offset history before the frame start", lambda: frame([compressed(lit_raw(noise(12, 115)), [(2, 3, 3)])], **WIN), verdict="invalid")
case("offset history across blocks of every kind",
     lambda: frame([raw(noise(16, 109)), compressed(_lits(_REPS[:3], 116), _REPS[:3]), compressed(lit_raw(noise(4, 117)), [(2, 3, 1), (1, 3, 2)]), compressed(lit_raw(noise(6, 118)), []),
                    raw(noise(5, 119)), rle(6, 7), compressed(lit_raw(noise(9, 120)), [(3, 3, 1), (1, 3, 2), (1, 3, 3), (0, 4, 3)])], **WIN),
     ["history_across_compressed", "history_across_zero_seq", "history_across_raw", "history_across_rle"])
case("offset below the match length", lambda: frame([compressed(lit_raw(noise(7, 121)), [(5, 40, off(3)), (1, 9, off(2))])], **WIN), ["offset_lt_ml"])
case("offset equal to the position", lambda: frame([compressed(lit_raw(noise(7, 122)), [(5, 3, off(5))])], **WIN), ["offset_eq_position"])
case("offset one past the position", lambda: frame([compressed(lit_raw(noise(7, 123)), [(5, 3, off(6))])], **WIN), verdict="invalid")
case("match reads a raw and an rle block",
     lambda: frame([raw(noise(20, 124)), rle(9, 20), compressed(lit_raw(noise(5, 125)), [(2, 10, off(35)), (1, 10, off(20))])], **WIN),
     ["match_reads_raw_block", "match_reads_rle_block"])
case("more literal lengths than literals", lambda: frame([raw(noise(20, 126)), compressed(lit_raw(noise(3, 127)), [(5, 3, off(1))])], **WIN),
     verdict="invalid")

# ---- record density -----------------------------------------------------------------------------------------------------------------
DENSE = "one sequence per three bytes"
case(DENSE, lambda: frame([compressed(lit_raw(b"\x17"), [(1, 3, off(1))] + [(0, 3, off(1))] * 21999)], **WIN), ["nbseq_2byte"], path="handed_back")
DENSE_COMPANION = "fcs 2 bytes, content 65791"  # with two of these in the call the record arena holds the dense frame's records


@lru_cache(maxsize=None)
def built(name: str):
    """(frame bytes, the bytes the writer's own execution of the sequences gives | None) of a case"""
    c = next(c for c in CASES if c["name"] == name)
    return build(c["spec"]())


def capacity(c) -> int:
    """the destination capacity a case is decoded with: its content (a near miss: what its sequences describe) and cap_extra"""
    _, out = built(c["name"])
    return (len(out) if out is not None else 64) + c["cap_extra"]


# ---- the feature list: every row needs a frame, crafted here or emitted by the reference encoder -----------------------------------
FEATURES = (
    ["single_segment", "fcs_1", "fcs_2", "fcs_4", "fcs_8", "fcs_1_content_255", "fcs_2_content_256", "fcs_2_content_65791", "window_with_fcs",
     "window_without_fcs", "checksum", "concatenated", "skippable_first", "skippable_after_frame", "skippable_last", "content_0"]
    + ["block_raw", "block_rle", "block_compressed", "last_raw", "last_rle", "last_compressed", "raw_block_empty_mid", "rle_block_131072",
       "compressed_block_131072"]
    + [f"lit_{m}_n{n}" for m in ("raw", "rle") for n in (31, 32, 4095, 4096)]
    + ["lit_huf_1stream_n1023", "lit_huf_4stream_n1024", "lit_huf_4stream_n16383", "lit_huf_4stream_n16384", "lit_huf_4stream_n6",
       "lit_huf_last_stream_empty", "huf_direct_odd", "huf_direct_even", "huf_two_symbols", "huf_max_bits_11", "huf_fse", "huf_stream_short",
       "huf_stream_long", "lit_treeless", "treeless_directly_after_tree", "treeless_after_raw_literals", "treeless_after_raw_rle_block"]
    + ["nbseq_0", "nbseq_1", "nbseq_127", "nbseq_128", "nbseq_32511", "nbseq_ge_0x7F00", "nbseq_1byte", "nbseq_2byte", "nbseq_3byte"]
    + [f"{t}_{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")]
    + ["repeat_after_predefined", "repeat_after_rle", "repeat_after_fse", "repeat_across_zero_seq_block", "repeat_across_raw_rle_block"]
    + [f"ll_code_{c}" for c in range(36)] + [f"ml_code_{c}" for c in range(53)] + [f"of_code_{c}" for c in range(24)]
    + ["offset_value_ge_2p24", "seq_bits_above_64", "seq_of_bits_0", "seq_ml_ll_bits_0", "of_codes_above_23_unused"]
    + [f"offset_value_{v}_{k}" for v in (1, 2, 3) for k in ("ll", "ll0")]
    + ["repeat1_minus_one", "initial_history_1_used", "initial_history_4_used", "initial_history_8_used", "initial_history_in_first_block",
       "history_across_compressed", "history_across_zero_seq", "history_across_raw", "history_across_rle", "offset_1_long_match", "offset_lt_ml",
       "offset_eq_position", "match_reads_raw_block", "match_reads_rle_block"]
)
# rows whose near miss (one step outside the format) is in CASES: feature -> case name.  The verdict is "invalid" but for one the
# reference decodes and only the decoders here refuse ("stricter"): 131073 bytes from one block
NEAR_MISSES = {
    "reserved bit": "reserved header bit", "dictionary": "dictionary id", "content size + 1": "content size one too large",
    "content size - 1": "content size one too small", "131073 from one block": "compressed block regenerates 131073", "block type 3": "block type 3",
    "block above the window": "compressed block larger than a single-segment frame's window", "4 streams of 5": "four streams of 5 literals",
    "treeless first": "treeless in the first block", "literal stream zero byte": "literal stream ends in a zero byte",
    "literal stream not consumed": "literal stream with a bit left over", "repeat first": "repeat in the first block",
    "LL log 10": "literal-length table log above its maximum", "OF log 9": "offset table log above its maximum",
    "ML log 10": "match-length table log above its maximum", "count short": "normalised count one short of its table",
    "bit-stream not consumed": "sequence bit-stream with a bit left over", "bit-stream zero byte": "sequence bit-stream ends in a zero byte",
    "reserved modes": "reserved mode bits", "repeat 1 - 1 = 0": "repeat 1 minus one is zero",
    "initial history too early": "initial offset history before the frame start", "position + 1": "offset one past the position",
    "literals exhausted": "more literal lengths than literals",
}
