"""The hand-built pieces of tests/zstd_encoder_units.py through the host instantiations of the zstd block encoder (oracle/zstd_model.c:
zstd_block_core.h with one lane; oracle/zstd_model_lanes.c: with 64), proved on the CPU to be what they claim.  For every case, in the
sub-block layout (zb_encode_piece_sub, the product's):
  - the piece, framed as ltz_model_compress frames it, decodes to the bytes its records execute to: with this library's decoder
    (ltz_model_decompress) and with the REFERENCE decoder (live where oracle/_ref is built, else its recorded answer);
  - the census of the frame (tests/zstd_format.py) holds every claimed key and none of the excluded ones;
  - literals read from the unit buffers and literals read from the source at every alignment 0 .. 3 give the same bytes (units without a
    sequence have no literal buffer on the GPU: theirs holds 0xA5 then); without a source no unit can be a Raw_Block, so there the
    bytes are only required to decode, and to be the same again when the case has no Raw unit;
  - 64 lanes in both orders write the one-lane bytes, and what the output buffer held before (0xA5, 0x00, 0xFF) changes nothing.
The one-block-per-piece layout and ZB_F_REPCODES run the same table and are checked for decoding only.  The union of the census over
the table holds every key this file lists as REACHABLE; UNREACHABLE names the others with the reason."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from tests import zstd_encoder_units as E
from tests import zstd_format as Z
from tests._libs import digest

IDS = [c["name"] for c in E.CASES]
_census = {}  # case name -> census of its sub-block frame (filled by test_case, read by the union tests)


@pytest.fixture(scope="module")
def model(oracle):
    d = oracle.dll
    d.ltz_model_encode_block_src.restype = C.c_uint32
    d.ltz_model_encode_block_src.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    d.ltz_model_last_sub.restype = C.POINTER(C.c_uint16)
    d.ltz_model_decompress.restype = C.c_int
    d.ltz_model_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    for name in ("ltz_model_sub_blocks", "ltz_model_lanes64", "ltz_model_fill"):
        getattr(d, name).restype = None
        getattr(d, name).argtypes = [C.c_int]
    d.ltz_model_flags.restype = None
    d.ltz_model_flags.argtypes = [C.c_uint32]
    yield d
    d.ltz_model_sub_blocks(0)
    d.ltz_model_lanes64(0)
    d.ltz_model_fill(0xA5)
    d.ltz_model_flags(0)


def encode(d, piece, sub=1, align=None, lanes=0, fill=0xA5, flags=0):
    """One piece through the model.  align None: no source, every unit's literals in its buffer; else the source stands at that
    address mod 4 and the units without a sequence have 0xA5 for a buffer.  Returns (size, bytes, directory entries)."""
    raw, meta, lits, recs = piece
    nunits = len(meta)
    src = None
    if align is not None:
        lits = lits.copy()
        lits[meta[:, 0] == 0] = 0xA5
        buf = np.full(len(raw) + 32, 0xEE, np.uint8)  # (aligned loads reach the words around the source: never beyond them)
        at = 8 + (align - buf.ctypes.data - 8) % 4
        buf[at : at + len(raw)] = raw
        src = buf.ctypes.data + at
        assert src % 4 == align
    out = np.full(140000, 0x77, np.uint8)
    d.ltz_model_sub_blocks(sub)
    d.ltz_model_lanes64(lanes)
    d.ltz_model_fill(fill)
    d.ltz_model_flags(flags)
    try:
        n = d.ltz_model_encode_block_src(meta.ctypes.data, lits.ctypes.data, recs.ctypes.data, nunits, len(raw), src, out.ctypes.data)
        subs = [int(d.ltz_model_last_sub()[u]) for u in range(nunits)] if sub else None
    finally:
        d.ltz_model_sub_blocks(0)
        d.ltz_model_lanes64(0)
        d.ltz_model_fill(0xA5)
        d.ltz_model_flags(0)
    assert n != 0xFFFFFFFF, "the 64 lanes did not keep step"
    assert n <= len(raw) + 2 and (out[n:] == 0x77).all()
    return n, out[:n].copy(), subs


def framed(raw, n, out, subs):
    """the frame ltz_model_compress makes of one piece: magic, single segment with an 8-byte content size, the piece's block(s)"""
    head = bytes([0x28, 0xB5, 0x2F, 0xFD, 0xE0]) + len(raw).to_bytes(8, "little")
    if n == 0:
        return np.frombuffer(head + (1 | len(raw) << 3).to_bytes(3, "little") + raw.tobytes(), np.uint8).copy()
    body = out.copy()
    if subs is None:
        return np.frombuffer(head + (1 | 2 << 1 | n << 3).to_bytes(3, "little") + body.tobytes(), np.uint8).copy()
    body[n - 3 - (subs[-1] & 0x7FFF)] |= 1  # Last_Block
    return np.frombuffer(head + body.tobytes(), np.uint8).copy()


def decodes(d, refcall, frame, raw, what):
    got = np.zeros(len(raw) + 8, np.uint8)
    n = C.c_size_t(0)
    assert d.ltz_model_decompress(frame.ctypes.data, len(frame), got.ctypes.data, len(raw), C.byref(n)) == 0, what
    assert n.value == len(raw) and (got[: n.value] == raw).all(), what

    def decode(r):
        err, back = r.decompress(1, frame, len(raw))
        return [int(err), len(back), digest(back)]

    assert refcall("zstd_decompress", [frame, len(raw)], decode) == [0, len(raw), digest(raw)], what


@pytest.mark.parametrize("case", E.CASES, ids=IDS)
def test_case(case, model, refcall):
    d = model
    piece = E.built(case["name"])
    raw, meta = piece[0], piece[1]
    # the product's form: the source at hand
    n, out, subs = encode(d, piece, align=0)
    assert (n == 0) == case["zero"], f"returns {n}: the piece is {'not ' if case['zero'] else ''}handed back"
    frame = framed(raw, n, out, subs)
    decodes(d, refcall, frame, raw, "source form")
    found = Z.census(bytes(frame))
    _census[case["name"]] = found
    if n:
        # the directory entries are the blocks the census walks
        assert sum((s & 0x7FFF) + 3 for s in subs) == n
        assert found["block_raw"] == sum(1 for s in subs if s & 0x8000) and found["block_compressed"] == sum(1 for s in subs if not s & 0x8000)
        missing = [k for k in case["has"] if not found[k]]
        present = [k for k in case["hasnt"] if found[k]]
        assert not missing and not present, f"claimed and not found: {missing}; excluded and found: {present}"
    for align in (1, 2, 3):
        n2, out2, _ = encode(d, piece, align=align)
        assert n2 == n and (out2 == out).all(), f"the source at address {align} mod 4 changes the bytes"
    # literals of every unit from its buffer (no source: no Raw units)
    n3, out3, subs3 = encode(d, piece, align=None)
    if n3:
        assert not any(s & 0x8000 for s in subs3)
        decodes(d, refcall, framed(raw, n3, out3, subs3), raw, "unit-buffer form")
    if n and not found["block_raw"]:
        assert n3 == n and (out3 == out).all(), "literals from the unit buffers and from the source give different bytes"
    # 64 lanes, both orders, and other fills
    for lanes in (1, 2):
        nl, outl, _ = encode(d, piece, align=1, lanes=lanes)
        assert nl == n and (outl == out).all(), f"64 lanes (order {lanes}) write other bytes than one lane"
    for fill, lanes in ((0x00, 0), (0xFF, 0), (0x00, 1), (0xFF, 2)):
        nf, outf, _ = encode(d, piece, align=2, lanes=lanes, fill=fill)
        assert nf == n and (outf == out).all(), f"the output depends on what the buffer held (fill {fill:#x}, lanes {lanes})"
    # the other layout and the repeat codes: decoding only
    nb, outb, _ = encode(d, piece, sub=0, align=0)
    decodes(d, refcall, framed(raw, nb, outb, None), raw, "one block per piece")
    nr, outr, subr = encode(d, piece, align=0, flags=1)
    decodes(d, refcall, framed(raw, nr, outr, subr), raw, "ZB_F_REPCODES")


# ---- what the table reaches --------------------------------------------------------------------------------------------------------------
REACHABLE = sorted(
    [f"lit_n{n}" for n in Z.LIT_COUNTS]
    + [f"lit_huf_n{n}" for n in (255, 256, 257, 258, 259, 260, 1023, 1024, 4092, 4095, 4096)]
    + ["lit_raw", "lit_raw_hdr1", "lit_raw_hdr2", "lit_raw_n31", "lit_raw_n32", "lit_huf_1stream", "lit_huf_4stream", "lit_huf_hdr3", "lit_huf_hdr4",
       "lit_huf_tree", "lit_treeless", "treeless_directly_after_tree", "treeless_after_raw_literals", "treeless_after_raw_rle_block",
       "lit_huf_4stream_n1023", "lit_huf_4stream_n1024", "lit_huf_4stream_last_shortest", "huf_block_without_sequences",
       "huf_direct", "huf_direct_odd", "huf_direct_even", "huf_fse", "huf_two_symbols"]
    + [f"huf_max_bits_{b}" for b in range(1, 12)]
    + [f"lit_huf_4stream_seg_mod16_{r}" for r in (0, 1, 4, 12, 11, 15)]
    + [f"nbseq_{n}" for n in (0, 1, 127, 128, 255, 256, 1023, 1024)] + ["nbseq_1byte", "nbseq_2byte"]
    + [f"{t}_{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")]
    + ["predefined_again", "repeat_after_fse", "repeat_after_rle", "repeat_directly", "repeat_across_zero_seq_block", "repeat_across_raw_rle_block"]
    + ["ll_fse_log_5", "ll_fse_log_9", "of_fse_log_5", "of_fse_log_8", "ml_fse_log_5", "ml_fse_log_6", "ml_fse_log_9",
       "ll_fse_several_count_1", "of_fse_several_count_1", "ml_fse_several_count_1"]
    + [f"ll_code_{c}" for c in range(31)] + [f"ml_code_{c}" for c in range(1, 48)] + [f"of_code_{c}" for c in range(2, 17)]
    + ["block_raw", "block_compressed", "last_raw", "last_compressed", "raw_block_first", "raw_block_mid", "raw_block_last",
       "raw_block_after_raw_block", "raw_block_after_compressed", "compressed_after_raw_block"]
    + [f"block_start_mod4_{r}" for r in range(4)]
    + [f"{s}_stream_start_mod4_{r}" for s in ("lit", "seq") for r in range(4)]
    + [f"{s}_stream_endbit_mod32_{b}" for s in ("lit", "seq") for b in range(32)])

UNREACHABLE = dict(E.UNREACHABLE_CODES)
UNREACHABLE.update({
    "lit_rle": "the encoder has no RLE literals mode (a piece of one literal value gets raw literals)",
    "block_rle": "zb_encode_piece_sub writes no RLE_Block: uniform pieces never reach it (k_zstd_scan writes them)",
    "lit_raw_hdr3": "raw literals of 4096 make a unit of 3 + 4096 + 1 bytes: it is a Raw_Block whenever the source is at hand",
    "lit_raw_n4095": "as lit_raw_hdr3: 2 + 4095 + 1 >= 4095 + the match bytes only if there are none, and then >= 4095",
    "lit_raw_n4096": "as lit_raw_hdr3",
    "lit_huf_hdr5": "a unit has at most 4096 literals: the 18-bit sizes are never needed",
    "nbseq_3byte": "a unit has at most 1024 sequences",
    "repeat_after_predefined": "Predefined_Mode is said again in every sub-block, never repeated",
    "lit_huf_last_stream_empty": "needs n - 3 * ((n + 3) >> 2) == 0: n = 3 or 6, far below the 256 literals four streams start at",
    "ll_fse_several_low_probability": "zb_normalize gives every present symbol a count >= 1: the encoder's own tables never hold the "
                                      "'less than one' probability (-1); only the predefined ones do (and so for of_, ml_)",
    "of_fse_several_low_probability": "as ll_fse_several_low_probability",
    "ml_fse_several_low_probability": "as ll_fse_several_low_probability",
    "offset_value_1_ll": "repeat codes only with ZB_F_REPCODES (checked for decoding, tests/test_zstd_model.py for the codes)",
})


def _need_all(d):
    """the census of every case (test_case leaves it behind; taken here for the cases that did not run)"""
    for c in E.CASES:
        if c["name"] not in _census:
            piece = E.built(c["name"])
            n, out, subs = encode(d, piece, align=0)
            _census[c["name"]] = Z.census(bytes(framed(piece[0], n, out, subs)))


def test_table_reaches_every_key_named_reachable(model):
    _need_all(model)
    total = Counter()
    for c in _census.values():
        total += c
    missing = [k for k in REACHABLE if not total[k]]
    assert not missing, f"no case holds {missing}"
    there = [k for k in UNREACHABLE if total[k]]
    assert not there, f"said to be unreachable, and found: {there}"


def test_alignment_sweep_ends_in_every_residue(model):
    """family (d): over the sweep every stream start (byte mod 4) and every stream end (bit mod 32) occurs, for the literal streams
    and for the sequence streams, the runs that end exactly on a word boundary among them; so does every block start mod 4"""
    _need_all(model)
    total = Counter()
    for c in E.CASES:
        if c["family"] == "d":
            total += _census[c["name"]]
    want = [f"{s}_stream_start_mod4_{r}" for s in ("lit", "seq") for r in range(4)] + [f"block_start_mod4_{r}" for r in range(4)]
    want += [f"{s}_stream_endbit_mod32_{b}" for s in ("lit", "seq") for b in range(32)]
    assert not [k for k in want if not total[k]], [k for k in want if not total[k]]


@pytest.mark.parametrize("ns", [127, 128])
def test_count_header_units_sit_on_the_raw_test(model, ns):
    """the two cases of E._count_header_piece stand where they say: at COUNT_HEADER_EDGE the probe unit is a Compressed_Block of
    ubytes - 1 bytes (lsize + shdr + sbytes: its tables were sent before), and so it is for the seven bits before it -- the last byte
    of its sequence stream is full --; one bit more and it is a Raw_Block: lsize + shdr + sbytes = ubytes"""
    edge = E.COUNT_HEADER_EDGE[ns]
    for more, want in [(edge - 8, E.U - 2), (edge - 7, E.U - 1), (edge, E.U - 1), (edge + 1, E.U | 0x8000)]:
        piece = E.execute_units(E._count_header_piece(ns, more))
        n, out, subs = encode(model, piece, align=0)
        assert n and subs[-1] == want, f"{ns} sequences, {more} bits: the unit's directory entry is {subs[-1]:#x}"
        found = Z.census(bytes(framed(piece[0], n, out, subs)))
        assert found["ll_fse_log_9"] and found["of_fse_log_8"] and found["ml_rle"] and (found[f"nbseq_{ns}"] > 0) == (want < 0x8000)


def test_families_are_all_there():
    n = Counter(c["family"] for c in E.CASES)
    assert set(n) == {"a", "b", "c", "d"} and n["d"] >= 64 and all(len(c["units"]) <= 32 for c in E.CASES)
