"""Hand-built PIECES for the zstd block encoder (zstd_block_core.h: zb_encode_piece_sub, the product's layout), given as the match finder
delivers them -- per 4 KiB unit meta {nseq, nlit, tail, uniform}, the unit's literal bytes and its records lit | ml << 16 | off << 32 --
so that every threshold of the entropy stage is hit exactly, with no match finder in the way.  The raw bytes of a piece are computed by
EXECUTING its records (execute_units).  Every case is named for the corner it holds and carries its CLAIMS: the census keys
(tests/zstd_format.py) the sub-block frame of the piece must contain (`has`) or must not contain (`hasnt`), or `zero`: the encoder
hands the piece back (returns 0: one Raw_Block).  Pure numpy; the encoder runs in tests/test_zstd_encoder_units_cases.py.

Where the thresholds are (zb_sub.h):
  phase 2   Huffman is tried when nlit >= 256 and largest > (nlit >> 7) + 4 (piece totals); no Huffman and fewer match bytes than
            3 * nbseq + 32: the piece is handed back; from 32768 literals a sampled histogram decides that earlier.
  phase 5   per unit: raw literals header 1 / 2 / 3 bytes for n < 32 / < 4096 / 4096; Huffman in one stream for n < 256, else four of
            seg = (n + 3) >> 2; header 3 bytes for n < 1024 and cs < 1024, else 4; sequence count in 1 byte for ns < 128, else 2;
            the unit is a Raw_Block when lsize + shdr + sbytes >= its bytes (only with the source at hand); the piece is handed back
            when all of it reaches raw_size + 3.
  tables    (zb_build_seq_tables) one code only: RLE; fewer than 64 sequences in the piece: Predefined; else FSE with accuracy log
            highbit(nbseq) - 1 clamped to [5 or 6, 9 / 8 / 9].

Codes that cannot occur, by the limits of a unit and of a record (UNREACHABLE_CODES): a unit has 4096 bytes and a sequence at least
4 match bytes, so a literal run in front of a match is at most 4092: LL code <= 30 (31 starts at 4096).  A match is 4 .. 4096 bytes:
ML code 0 is length 3, code 48 starts at 4099.  An offset is 1 .. 65535 and, without repeat codes, goes out as offset + 3 =
4 .. 65538: OF code 2 .. 16 (0 and 1 are the repeat values 1 .. 3, 17 starts at 131072)."""
from __future__ import annotations

import functools

import numpy as np

U = 4096
SEQ_MAX = 1024
LL_EDGES = [(c, b, b + (1 << nb) - 1) for c, (b, nb) in enumerate(zip(
    list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048],
    [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11]))]  # (code, smallest, largest literal run) for LL codes 0 .. 30
ML_EDGES = [(c, b, b + (1 << nb) - 1) for c, (b, nb) in enumerate(zip(
    list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051],
    [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11]))][1:]  # ML codes 1 .. 47 (code 47 ends at 4096 in a unit)
OF_EDGES = [(c, (1 << c) - 3, min((2 << c) - 4, 65535)) for c in range(2, 17)]  # OF codes 2 .. 16: offsets 1 .. 65535
UNREACHABLE_CODES = {
    "ll_code_31": "a unit with a sequence holds at most 4092 literals, code 31 starts at 4096 (and so for codes 32 .. 35)",
    "ml_code_0": "the shortest match of a record is 4 bytes, code 0 is 3",
    "ml_code_48": "a match ends with its unit: at most 4096 bytes, code 48 starts at 4099 (and so for codes 49 .. 52)",
    "of_code_0": "plain offsets go out as offset + 3 >= 4 (code 2); codes 0 and 1 are the repeat values (ZB_F_REPCODES only)",
    "of_code_1": "as of_code_0",
    "of_code_17": "an offset is at most 65535: offset + 3 < 131072 (and so for codes 18 .. 31)",
}


def execute_units(units):
    """units: per unit (seqs, tail) with seqs = [(literal bytes, match length, offset)] and tail = the literal bytes behind the last
    match.  Executes the sequences into the raw bytes they describe and returns (raw, meta, lits, recs) as the match finder delivers
    them.  Every unit is 4096 bytes, the last one may be shorter."""
    nunits = len(units)
    raw = bytearray()
    meta = np.zeros((nunits, 4), np.uint32)
    lits = np.zeros((nunits, U), np.uint8)
    recs = np.zeros((nunits, SEQ_MAX), np.uint64)
    for u, (seqs, tail) in enumerate(units):
        start, nlit = len(raw), 0
        assert start == u * U and len(seqs) <= SEQ_MAX, "a unit before the last one is 4096 bytes"
        for k, (lit, ml, off) in enumerate(seqs):
            lit = bytes(lit)
            raw += lit
            lits[u, nlit : nlit + len(lit)] = np.frombuffer(lit, np.uint8)
            nlit += len(lit)
            # (the match finder's matches are 4 bytes and more; the format's shortest is 3)
            assert 3 <= ml <= U and 1 <= off <= min(len(raw), 65535), (u, k, ml, off, len(raw))
            if off >= ml:
                raw += raw[len(raw) - off : len(raw) - off + ml]
            else:  # overlapping: the period repeats
                pat = bytes(raw[len(raw) - off :])
                raw += (pat * (ml // off + 1))[:ml]
            recs[u, k] = len(lit) | (ml << 16) | (off << 32)
        tail = bytes(tail)
        raw += tail
        lits[u, nlit : nlit + len(tail)] = np.frombuffer(tail, np.uint8)
        nlit += len(tail)
        assert len(raw) - start == U or (u == nunits - 1 and 0 < len(raw) - start < U), (u, len(raw) - start)
        meta[u] = (len(seqs), nlit, len(tail), 0)
    return np.frombuffer(bytes(raw), np.uint8).copy(), meta, lits, recs


# ---- ingredients ----------------------------------------------------------------------------------------------------------------------
class Lit:
    """literal bytes of one distribution, drawn in order from one seeded stream"""

    def __init__(self, seed, kind="skew"):
        self.rng, self.kind = np.random.default_rng(seed), kind

    def __call__(self, n):
        if self.kind == "skew":  # about 5.5 bits a byte: Huffman pays
            return ((np.abs(self.rng.normal(100, 12, n)).astype(np.int64)) % 256).astype(np.uint8).tobytes()
        if self.kind == "noise":
            return self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        if self.kind == "two":
            return self.rng.choice(2, n, p=[0.85, 0.15]).astype(np.uint8).tobytes()
        if self.kind == "one":
            return b"\x41" * n
        raise KeyError(self.kind)


def pack(items, lit, size=None):
    """items: (literals in front, match length, offset) triples, or None: the unit ends here.  Fills units in order; a unit's rest is
    tail literals.  size: the piece's bytes (the last unit is cut or filled to it), default: whole units."""
    units, seqs, used = [], [], 0

    def close(fill=U):
        nonlocal seqs, used
        units.append((seqs, lit(fill - used)))
        seqs, used = [], 0

    for it in items:
        if it is None:
            close()
            continue
        n, ml, off = it
        if used + n + ml > U or len(seqs) == SEQ_MAX:
            close()
        seqs.append((lit(n), ml, off))
        used += n + ml
    if size is None:
        if used or seqs or not units:
            close()
    else:
        rest = size - len(units) * U
        assert used <= rest <= U and rest > 0, (size, len(units), used)
        close(rest)
    return units


def plain(lit, n=U):
    """a unit without a sequence: n literal bytes"""
    return ([], lit(n))


def one_seq(lit, n, off, front=None):
    """a whole unit of n literals and one match of the rest: `front` of the literals stand in front of the match (default: all)"""
    front = n if front is None else front
    return ([(lit(front), U - n, off)], lit(n - front))


_CASES = []


def case(family, name, units, has=(), hasnt=(), zero=False, note=""):
    _CASES.append(dict(family=family, name=name, units=units, has=tuple(has), hasnt=tuple(hasnt), zero=zero, note=note))


HUF = ("lit_huf_tree",)
NO_HUF = ("lit_huf_tree", "lit_treeless", "lit_huf_1stream", "lit_huf_4stream")


def _counts_bytes(counts, seed):
    """bytes with exactly counts[s] of symbol s, shuffled"""
    b = np.concatenate([np.full(c, s, np.uint8) for s, c in counts.items()])
    np.random.default_rng(seed).shuffle(b)
    return b.tobytes()


# ---- (a) the literals section ----------------------------------------------------------------------------------------------------------
def _family_a():
    # per-unit literal counts: a plain unit in front (the matches need history), the probe unit(s), a unit that keeps the piece paying
    probes = [(0, ("lit_n0",)), (1, ("lit_n1",)), (31, ("lit_n31",)), (32, ("lit_n32",)), (255, ("lit_huf_n255", "lit_huf_1stream")),
              (256, ("lit_huf_n256", "lit_huf_4stream")), (257, ("lit_huf_n257", "lit_huf_4stream_last_shortest")), (258, ("lit_huf_n258",)),
              (259, ("lit_huf_n259",)), (260, ("lit_huf_n260",)), (1023, ("lit_huf_4stream_n1023", "lit_huf_hdr3")),
              (1024, ("lit_huf_4stream_n1024", "lit_huf_hdr4")), (4092, ("lit_huf_n4092",))]
    for n, has in probes:
        for front in ([None] if n < 2 else [None, n // 2]):
            lit = Lit(1000 + n)
            units = [plain(lit), one_seq(lit, n, U if n else 7, front), one_seq(lit, 300, 2 * U + 5)]
            where = "all in front of the match" if front is None else "half in front of the match, half behind it"
            case("a", f"a unit of {n} literals, {where}", units, has + HUF)
    for n, last in ((4095, 4095), (4096, 4096)):
        lit = Lit(1100 + n)
        case("a", f"{n} literals and no sequence in the last unit of a piece", [plain(lit), one_seq(lit, 500, U), plain(lit, last)],
             (f"lit_huf_n{n}", "huf_block_without_sequences", "lit_huf_hdr4") + HUF)
    for n in (301, 333, 1001, 2049, 4089):  # seg = 76, 84, 251, 513, 1023: multiples of 4 but not of 16, and odd
        lit = Lit(1200 + n)
        seg = (n + 3) >> 2
        units = [plain(lit), ([(lit(n - 100), U - n, 77)], lit(100)), plain(lit, n)]
        case("a", f"four streams of {seg} literals (n = {n}), read from the unit and from the source", units,
             (f"lit_huf_4stream_seg_mod16_{seg & 15}",) + (("lit_huf_4stream_last_shortest",) if n % 4 == 1 else ()) + HUF)
    # the Huffman decision largest > (nlit >> 7) + 4: 64 symbols, four of each but symbol 0
    for nlit, largest, tried in ((256, 5, False), (256, 6, False), (256, 7, True), (255, 7, False), (255, 6, False)):
        counts = {s: 4 for s in range(64)}
        counts[0] = largest
        for s in range(1, 1 + largest - 4 + (256 - nlit)):
            counts[s] -= 1
        assert sum(counts.values()) == nlit and max(counts.values()) == largest
        data = _counts_bytes(counts, 7)
        case("a", f"{nlit} literals, the most frequent {largest} times: Huffman {'tried' if tried else 'not tried'}",
             [([], data)], (HUF + ("huf_block_without_sequences",)) if tried else (),
             () if tried else NO_HUF, zero=not tried, note="threshold (nlit >> 7) + 4 = " + str((nlit >> 7) + 4))
    # the same decision with the piece's literals spread over two units (the counts are the piece's, the streams the units')
    counts = {s: 8 for s in range(64)}
    counts[0] = 9
    counts[1] = 7
    data = _counts_bytes(counts, 8)  # 512 literals, threshold 8: tried at 9
    lit = Lit(3)
    case("a", "512 literals over three units, the most frequent 9 times: Huffman tried, one stream each",
         [([(data[:200], U - 200, 200)], b""), ([(data[200:300], U - 200, U)], data[300:400]), ([(data[400:], U - 112, U)], b"")],
         ("lit_huf_1stream", "lit_treeless") + HUF, ("lit_huf_4stream", "lit_raw"))
    # tree shapes
    lit = Lit(21, "two")
    case("a", "two symbols", [plain(lit), one_seq(lit, 900, U)], ("huf_two_symbols", "huf_max_bits_1", "huf_direct") + HUF)
    lit = Lit(22, "one")
    case("a", "one symbol only (units not uniform): no tree exists, raw literals",
         [([(lit(300), U - 300, 300)], b""), one_seq(lit, 400, U)], ("lit_raw",), NO_HUF)
    for top, key in ((127, "huf_direct"), (128, "huf_direct"), (129, "huf_fse"), (255, "huf_fse")):
        rng = np.random.default_rng(top)
        b = np.minimum(rng.geometric(0.06, 6000) - 1, top).astype(np.uint8)
        b[: top + 1] = np.arange(top + 1).astype(np.uint8)  # (every symbol up to the largest occurs)
        b = b.tobytes()
        case("a", f"largest literal symbol {top}: {'direct' if key == 'huf_direct' else 'FSE-coded'} weights",
             [([], b[:U]), ([(b[U:6000], 2 * U - 6000, U)], b"")], (key,) + HUF)
    for bits in range(1, 12):
        counts = {0: 1, 1: 1}
        for s in range(2, bits + 1):
            counts[s] = 1 << (s - 1)
        scale = max(1, -(-320 // sum(counts.values())))
        data = _counts_bytes({s: c * scale for s, c in counts.items()}, bits)
        assert len(data) <= U
        case("a", f"deepest Huffman code {bits} bits", [([], data)], (f"huf_max_bits_{bits}", "huf_block_without_sequences") + HUF)
    rng = np.random.default_rng(5)
    deep = np.minimum(rng.geometric(0.5, 3 * U) - 1, 40).astype(np.uint8).tobytes()
    case("a", "depths far above 11 cut to the limit", [([], deep[:U]), ([], deep[U : 2 * U]), ([], deep[2 * U :])], ("huf_max_bits_11",) + HUF)
    # a tree that cannot be described: 254 symbols of 8 bits, symbol 254 of 7 -- weights 1 .. 1 for symbols 0 .. 253 are more than 128
    # weights (FSE-coded) of ONE value, which FSE cannot code
    data = _counts_bytes({**{s: 10 for s in range(254)}, 254: 30}, 9)
    case("a", "a tree whose description fails (254 equal weights): raw literals",
         [([(data, U - len(data), len(data))], b"")], ("lit_raw",), NO_HUF, note="largest 30 > (2570 >> 7) + 4 = 24: Huffman is tried")
    # the noise tests
    noise = Lit(31, "noise")
    case("a", "units of 31 and 32 literals of noise: raw literals with the 1-byte and the 2-byte header",
         [plain(noise), one_seq(noise, 31, U), one_seq(noise, 32, U), one_seq(noise, 0, 3)],
         ("lit_raw_n31", "lit_raw_n32", "lit_raw_hdr1", "lit_raw_hdr2", "raw_block_first"), NO_HUF)
    case("a", "32768 literals of noise: the sampled test hands the piece back", [plain(noise) for _ in range(8)], zero=True)
    case("a", "32767 literals of noise: not sampled, phase 2 hands the piece back", [plain(noise) for _ in range(7)] + [plain(noise, U - 1)], zero=True)
    two = Lit(32, "two")
    case("a", "32768 literals, the sampled unit skewed, the others noise: Huffman, Raw_Blocks for the noise",
         [plain(two)] + [plain(noise) for _ in range(7)], ("raw_block_after_compressed", "raw_block_last") + HUF)
    m = [(0, 8, 900)] * 500  # 4000 match bytes >= 3 * 500 + 32
    case("a", "32864 literals of noise, enough match bytes: not sampled away, raw literals",
         [plain(noise) for _ in range(8)] + pack(m, noise), ("lit_raw", "raw_block_first", "raw_block_after_raw_block", "ll_rle"), NO_HUF)
    rng = np.random.default_rng(33)
    # the sample is the whole first unit (4096 bytes): every one of 128 values stands 32 times in it, 32 <= (4096 >> 7) + 4 = 36
    flat = rng.permutation(np.arange(2048, dtype=np.int64) % 128).astype(np.uint8).tobytes()
    case("a", "the sampled unit flat over 128 symbols (largest 32 <= (4096 >> 7) + 4): handed back",
         [([], flat + flat)] + [plain(noise) for _ in range(7)], zero=True)
    # ... and at equality and one above: 128 values 32 times each but for the most frequent one; the other seven units hold two values, so
    # that a piece that is not handed back shows it (Huffman is built; the flat unit is a Raw_Block)
    for largest, back in ((36, True), (37, False)):
        counts = {s: 32 for s in range(128)}
        counts[0] = largest
        for s in range(1, 1 + largest - 32):
            counts[s] -= 1
        assert sum(counts.values()) == U and max(counts.values()) == largest
        case("a", f"the sampled unit's most frequent value {largest} times in 4096, (4096 >> 7) + 4 = 36, the other units of two values: "
             f"{'handed back' if back else 'kept'}", [([], _counts_bytes(counts, 34))] + [plain(two) for _ in range(7)],
             () if back else HUF + ("raw_block_first",), zero=back)
    # phase 2's own test (ZV_SKIP) each side: no Huffman, match bytes 3 * nbseq + 32 and one less
    for short in (0, 1):
        items = [(0, 4, 100)] * 30 + [(0, 5 - short, 100)]  # 31 sequences: 125 - short match bytes against 3 * 31 + 32 = 125
        case("a", f"noise with {125 - short} match bytes in 31 sequences: {'handed back' if short else 'kept'}",
             [plain(noise)] + pack(items, noise), () if short else ("lit_raw",), () if short else NO_HUF, zero=bool(short),
             note="kept: raw_size - nlit >= 3 * nbseq + 32")


# ---- (b) the sequences section ---------------------------------------------------------------------------------------------------------
def _family_b():
    for ns in (1, 127, 128, 255, 256, 1023, 1024):
        lit = Lit(2000 + ns)
        rng = np.random.default_rng(ns)
        items = [(int(rng.integers(0, 2)) if ns < 1023 else (1 if k < U - 4 * ns else 0), 4 + (int(rng.integers(0, 5)) if ns < 512 else 0),
                  int(rng.integers(4, 3000))) for k in range(ns)]
        used = sum(a + b for a, b, _ in items)
        assert used <= U
        seqs = [(lit(a), b, o) for a, b, o in items]
        case("b", f"a unit of {ns} sequences", [plain(lit), (seqs, lit(U - used)), one_seq(lit, 200, 9)], (f"nbseq_{ns}", "nbseq_0"))
    lit = Lit(2100)
    case("b", "the first two units have no sequence: the tables go out with the third",
         [plain(lit), plain(lit)] + pack([(3, 9, 4000 + k) for k in range(100)], lit) + [one_seq(lit, 50, 33)],
         ("nbseq_0", "ll_fse", "repeat_directly", "treeless_directly_after_tree"))
    case("b", "Repeat_Mode across a unit without a sequence",
         [plain(lit)] + pack([(k % 7, 5 + k % 9, 300 + 7 * k) for k in range(90)], lit) + [plain(lit)] + pack([(2, 6, 500)] * 5, lit),
         ("repeat_across_zero_seq_block", "repeat_after_fse"))
    case("b", "no sequence in the whole piece, Huffman pays", [plain(lit), plain(lit), plain(lit, 1000)],
         ("huf_block_without_sequences", "lit_treeless") + HUF, ("ll_fse", "ll_predefined", "ll_rle"))
    # modes
    case("b", "Predefined tables, and Predefined again in the later units",
         [plain(lit)] + pack([(1, 5, 100), (17, 40, 2000), None, (0, 4, 9), (3, 300, 4500), None, (2, 7, 5)], lit),
         ("ll_predefined", "of_predefined", "ml_predefined", "predefined_again"), ("ll_repeat", "ll_fse"))
    case("b", "every sequence has the same three codes: RLE tables, Repeat_Mode after them",
         [plain(lit)] + pack([(2, 6, 1500 + k) for k in range(70)] + [None] + [(2, 6, 1100)] * 9, lit),
         ("ll_rle", "of_rle", "ml_rle", "repeat_after_rle"))
    case("b", "one literal-length code but several offset and match codes: RLE beside FSE",
         [plain(lit)] + pack([(0, 4 + k % 30, 3 + 37 * k) for k in range(200)], lit), ("ll_rle", "of_fse", "ml_fse"))
    rng = np.random.default_rng(7)
    few = [(int(rng.integers(0, 3)), int(rng.integers(4, 8)), int(rng.integers(100, 120))) for _ in range(58)]
    rare = [(16 + 3 * k, 36 + 5 * k, 1 << (3 + k)) for k in range(6)]  # six codes of each kind that occur once
    case("b", "64 sequences, several symbols that occur once: FSE with the smallest accuracy log (5), counts of 1 and none of -1",
         [plain(lit), plain(lit)] + pack(few + rare, lit),
         ("ll_fse_log_5", "of_fse_log_5", "ml_fse_log_5", "ll_fse_several_count_1", "of_fse_several_count_1", "ml_fse_several_count_1"),
         ("ll_fse_several_low_probability", "of_fse_several_low_probability", "ml_fse_several_low_probability"),
         note="zb_normalize gives a symbol that occurs once the count 1, never the 'less than one' of the format (-1)")
    many = [(int(rng.integers(0, 4)), int(rng.integers(4, 12)), int(rng.integers(1, 4000))) for _ in range(1100)]
    case("b", "1100 sequences: FSE with the largest accuracy logs (9, 8, 9)", [plain(lit)] + pack(many + rare, lit),
         ("ll_fse_log_9", "of_fse_log_8", "ml_fse_log_9", "nbseq_2byte"))
    wide = [(k % 3, v, 100 + k) for k, v in enumerate((list(range(4, 35)) + [35, 37, 39, 41]) * 2)]  # 35 match-length codes, twice
    case("b", "70 sequences over more than 32 match-length codes: accuracy log 6", [plain(lit)] + pack(wide, lit), ("ml_fse_log_6",))
    # code ranges, both ends of every code
    ll = [(v, 4, 50) for c, lo, hi in LL_EDGES for v in sorted({lo, min(hi, U - 4)})]
    case("b", "every literal-length code 0 .. 30 at both ends of its range", [plain(lit)] + pack(ll, lit),
         tuple(f"ll_code_{c}" for c in range(31)), ("ll_code_31",))
    ml = [(0, v, 50) for c, lo, hi in ML_EDGES for v in sorted({lo, min(hi, U)})]
    case("b", "every match-length code 1 .. 47 at both ends of its range (4 .. 4096 bytes)", [plain(lit)] + pack(ml, lit),
         tuple(f"ml_code_{c}" for c in range(1, 48)), ("ml_code_0", "ml_code_48"))
    of = [(1, 5, v) for c, lo, hi in OF_EDGES for v in sorted({lo, hi})]
    case("b", "every offset code 2 .. 16 at both ends of its range (1 .. 65535)", [plain(lit) for _ in range(16)] + pack(of, lit),
         tuple(f"of_code_{c}" for c in range(2, 17)), ("of_code_0", "of_code_1", "of_code_17"))
    case("b", "the largest extra-bit values together: 4092 literals, then 4096 bytes from 65535 back",
         [plain(lit) for _ in range(16)] + [([(lit(U - 4), 4, 65535)], b""), ([(b"", U, 65535)], b""), one_seq(lit, 2047, 65534)],
         ("ll_code_30", "ml_code_47", "of_code_16", "lit_n0"))


# ---- (c) what a unit becomes -----------------------------------------------------------------------------------------------------------
def _raw_probe(lit, ml, size=U):
    """noise literals and ONE sequence of `ml` bytes at offset 4093 in RLE-mode tables (no state bits: 12 offset bits + the end mark =
    2 bytes): lsize + shdr + sbytes = (2 + size - ml) + 2 + 2 against size -- equal at ml = 6; with 31 literals and fewer the literals
    header is one byte: equal at ml = 5"""
    return ([(lit(2), ml, 4093)], lit(size - 2 - ml))


def _count_header_piece(ns, more):
    """The Raw_Block test where the sequence count's header grows (ns < 128: one byte, else two).  RLE tables cannot bring a unit of
    127 or 128 sequences there -- without state bits a sequence costs at most 18 bits against its 4 match bytes --, so the probe unit's
    sequences are made dear: sixteen units of 1024 sequences (no literals, 4 bytes from 8 back) make every code of the probe rare in
    the piece's tables (accuracy logs 9 and 8; the match lengths are all 4: RLE), and a code that zb_normalize gives the count 1 costs
    the whole accuracy log.  The probe's ns sequences have 1 .. 16 literals in front (eight of each: 16 literal-length codes) and
    offsets of the codes 13 .. 16, about 32 of each: 9 + 8 state bits and 13 .. 16 (+ 1 for 16 literals) extra bits a sequence.  `more`
    moves that many sequences from offset code 13 to 14 (negative: from 14 to 13): one bit each, with the same literals and the same
    match bytes.  lsize + shdr + sbytes - ubytes = 2 + (3 or 2) + sbytes - 4 * ns, the noise literals being raw."""
    noise = Lit(3200 + ns, "noise")
    bulk = pack([(8 if k == 0 else 0, 4, 8) for k in range(16 * SEQ_MAX - 2)], noise)
    assert len(bulk) == 16
    codes = [13] * 32 + [14] * 32 + [15] * 32 + [16] * 32
    for k in range(abs(more)):
        codes[k if more > 0 else 32 + k] = 14 if more > 0 else 13
    offs = {13: 8192, 14: 16384, 15: 32768, 16: 65533}
    seqs = [(noise(1 + k % 16), 4, offs[codes[k]]) for k in range(ns)]
    return bulk + [(seqs, noise(U - sum(len(l) + 4 for l, _, _ in seqs)))]


# `more` of _count_header_piece at which lsize + shdr + sbytes is one below the unit's 4096 bytes with the last bit of its last byte
# used: one bit more and it is 4096.  (Found by running the model over more = -24 .. 24: the unit's block is 4095 bytes up to here
# and a Raw_Block from the next on; tests/test_zstd_encoder_units_cases.py holds the two sizes.)
COUNT_HEADER_EDGE = {128: 7, 127: 17}


def _family_c():
    for ns in (128, 127):
        for step, raw in ((0, False), (1, True)):
            case("c", f"a unit of {ns} sequences (count in {'two bytes' if ns >= 128 else 'one byte'}) with lsize + shdr + sbytes = ubytes"
                 f"{'' if raw else ' - 1'}: {'a Raw_Block' if raw else 'compressed'}", _count_header_piece(ns, COUNT_HEADER_EDGE[ns] + step),
                 ("raw_block_last", "last_raw") if raw else ("last_compressed",), () if raw else ("raw_block_last",),
                 note="with ns <= 128 for ns < 128 in the size estimate the Raw unit of 128 stays compressed.  (The claims are the unit's "
                      "kind alone: the sequence count and the tables' modes are the match finder's on real bytes, and are held in "
                      "test_count_header_units_sit_on_the_raw_test)")
    for ml, raw in ((5, True), (6, True), (7, False)):
        lit = Lit(3000 + ml, "noise")
        others = pack([(2, ml, 4093)] * 200, lit)  # (the same three codes throughout: RLE tables; enough match bytes to keep the piece)
        case("c", f"lsize + shdr + sbytes = ubytes {'+ 1' if ml == 5 else '' if ml == 6 else '- 1'}: the unit is "
             f"{'a Raw_Block' if raw else 'compressed'}", [plain(lit)] + others + [_raw_probe(lit, ml)],
             ("ll_rle", "of_rle", "ml_rle") + (("raw_block_last",) if raw else ("last_compressed",)), () if raw else ("raw_block_last",),
             note="the first unit (no sequence, raw literals) is a Raw_Block in every one of the three")
    # the same at the literal counts where the raw literals header grows: the last unit has n literals and the one match
    for n, ml, raw in ((31, 5, True), (31, 6, False), (32, 6, True), (32, 7, False)):
        lit = Lit(3050 + n + ml, "noise")
        case("c", f"a last unit of {n} raw literals and a match of {ml}: lsize + shdr + sbytes = ubytes{'' if raw else ' - 1'}, "
             f"{'a Raw_Block' if raw else 'compressed'}", [plain(lit)] + pack([(2, ml, 4093)] * 200, lit) + [_raw_probe(lit, ml, n + ml)],
             ("raw_block_last", "last_raw") if raw else ("last_compressed", f"lit_raw_n{n}", f"lit_raw_hdr{1 if n < 32 else 2}"),
             () if raw else ("raw_block_last",), note=f"literals header {1 if n < 32 else 2} byte(s) + {n} + 2 + 2 against {n + ml}")
    skew, noise = Lit(3100), Lit(3101, "noise")

    def seqs(first=False, n=80):
        """a unit of 80 sequences; the piece's first unit begins with 1300 literals for its matches to reach back into"""
        return pack([((1300 if first and k == 0 else 0) + 3 + k % 5, 6 + k % 11, 200 + 13 * k) for k in range(n)], skew)

    case("c", "a Raw unit first: the tree and the tables are still due", [plain(noise)] + seqs() + seqs(),
         ("raw_block_first", "compressed_after_raw_block", "ll_fse", "repeat_directly") + HUF)
    case("c", "a Raw unit in the middle, tree and tables already sent: both live on across it", seqs(True) + [plain(noise)] + seqs(),
         ("raw_block_mid", "raw_block_after_compressed", "repeat_across_raw_rle_block", "treeless_after_raw_rle_block"))
    case("c", "a Raw unit in the middle, the tree sent and the tables still due", [plain(skew), plain(noise)] + seqs() + seqs(),
         ("raw_block_mid", "treeless_after_raw_rle_block", "ll_fse"), ("repeat_across_raw_rle_block",))
    case("c", "a Raw unit last (Last_Block on a Raw sub-block)", seqs(True) + seqs() + [plain(noise)], ("raw_block_last", "last_raw"))
    case("c", "two Raw units in a row", seqs(True) + [plain(noise), plain(noise)] + seqs(),
         ("raw_block_after_raw_block", "repeat_across_raw_rle_block", "treeless_after_raw_rle_block"))
    case("c", "Raw units first and last, a compressed one between (Last_Block on a partial Raw sub-block)",
         [plain(noise)] + seqs() + [plain(noise, 77)], ("raw_block_first", "raw_block_last", "last_raw"))
    for rest in (1, 8, 4095):  # (1 and 8 literals cost more than they are: 1 + n + 1 >= n)
        case("c", f"the last unit has {rest} literal bytes: {'compressed' if rest > 8 else 'a Raw_Block'}", [plain(skew)] + seqs() + [plain(skew, rest)],
             ("last_compressed", "huf_block_without_sequences", "lit_n4095") if rest > 8 else ("last_raw", "raw_block_last"))
    case("c", "a piece of 4097 bytes", [plain(skew), plain(skew, 1)], ("last_raw",) + HUF)
    for rest in (8, 4095):
        case("c", f"a last unit of {rest} bytes that is one match (Last_Block on a compressed sub-block)",
             seqs(True) + [([(b"", rest, 700)], b"")], ("last_compressed", "lit_n0", "nbseq_1"))
    rng = np.random.default_rng(9)
    # three sequences of 4 bytes at 15 offset bits each and the states cost 8 bytes and 4 of headers for 12: the unit is a Raw_Block
    costly = [it for _ in range(11) for it in [(0, 4, int(rng.integers(32768, 65533)))] * 3 + [None]]
    case("c", "every unit a Raw_Block though the piece passed the noise tests: the total reaches raw_size + 3, handed back",
         [plain(noise) for _ in range(16)] + pack(costly, noise), zero=True, note="132 match bytes >= 3 * 33 + 32")


# ---- (d) the staged output at every alignment ---------------------------------------------------------------------------------------------
SWEEP = 32


def _probe(lit, nl, nsq, first_off):
    """a unit of nl literals (four Huffman streams) and nsq + 1 sequences, the last one a match that fills the unit"""
    seqs = [(2 + j % 3, 5 + j % 7, 100 + 31 * j) for j in range(nsq)]
    seqs[0] = (2, 5, first_off)
    body, s, at = lit(nl), [], 0
    for a, b, o in seqs:
        s.append((body[at : at + a], b, o))
        at += a
    s.append((b"", U - sum(a + b for a, b, _ in seqs) - (nl - at), 4000))
    return (s, body[at:])


def _family_d():
    for k in range(SWEEP):
        for what in ("literal", "sequence"):
            lit = Lit(4000)  # (the same bytes in every case: one literal / one sequence more is all that changes)
            nl, nsq = (700 + k, 40) if what == "literal" else (700, 40 + k)
            front = ([(lit(20 + (k & 3)), U - 20 - (k & 3), 20 + (k & 3))], b"")  # block size over all residues mod 4
            lit = Lit(4001)
            units = [front, _probe(lit, nl, nsq, 100)]
            if what == "sequence":  # (two more probes whose first offset has other bit counts: more stream ends per case)
                units += [_probe(lit, 300 + k, nsq, 100 << (1 + k % 5)), _probe(lit, 300, nsq + 1, 100 << (k % 3))]
            case("d", f"{what} stream {k} longer behind a unit of residue {k & 3}", units,
                 ("lit_huf_4stream", "ll_predefined" if len(units) == 2 and nsq + 2 < 64 else "ll_fse"))


def _table():
    """the table, drawn up at its first use (a module that only wants execute_units does not pay for it)"""
    if not _CASES:
        _family_a()
        _family_b()
        _family_c()
        _family_d()
        assert len({c["name"] for c in _CASES}) == len(_CASES)
    return _CASES


def __getattr__(name):  # (the module has no global CASES: E.CASES comes here)
    if name == "CASES":
        return _table()
    raise AttributeError(name)


@functools.lru_cache(maxsize=None)
def built(name):
    """(raw, meta, lits, recs) of a case: the records executed"""
    c = next(c for c in _table() if c["name"] == name)
    return execute_units(c["units"])
