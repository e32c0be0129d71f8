"""The zstd frame format (RFC 8878) in plain Python: a census that says which format features a frame contains, and a writer that
builds frames from an explicit description -- every header form, block type, literals form, table mode, code and offset form, and
frames that are wrong on purpose.  tests/zstd_format_frames.py holds the case table built with it, tests/test_zstd_format_cases.py
proves on the CPU that the cases are what they claim, tests/test_gpu_zstd_format.py sends them through every way the GPU decodes.

Nothing here loads the library under test or restates an existing decoder: the tables, orders and bit layouts are the RFC's
(section numbers in the comments).  The writer computes the bytes a frame regenerates by executing its own sequences."""
from __future__ import annotations

from collections import Counter

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 1 << 17

# 3.1.1.3.2.1.1: literal-length and match-length codes -> (baseline, extra bits)
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _bases(first, bits):
    out, v = [], first
    for b in bits:
        out.append(v)
        v += 1 << b
    return out


LL_BASE = _bases(0, LL_BITS)  # 0 .. 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, ... 65536
ML_BASE = _bases(3, ML_BITS)  # 3 .. 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, ... 65539
# 3.1.1.3.2.2: the predefined distributions (accuracy logs 6, 5, 6)
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
LL, OF, ML = 0, 1, 2
NAMES = ("ll", "of", "ml")
LIT_COUNTS = (0, 1, 31, 32, 255, 256, 257, 258, 259, 260, 1023, 1024, 4092, 4095, 4096)  # the literal counts the census names (lit_n*)
DEFAULTS = ((LL_DEFAULT, 6), (OF_DEFAULT, 5), (ML_DEFAULT, 6))
MAX_LOG = (9, 8, 9)
MAX_SYM = (35, 31, 52)
MODES = ("predefined", "rle", "fse", "repeat")


class FormatError(Exception):
    """the census met something the format does not allow (or a truncated frame)"""


def code_of(bases, v):
    c = len(bases) - 1
    while bases[c] > v:
        c -= 1
    return c


# ---- XXH64 (the content checksum, 3.1.1: its low four bytes) ----------------------------------------------------------------------
_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _xround(acc, lane):
    return _rotl((acc + lane * _P2) & _M, 31) * _P1 & _M


def xxh64(data: bytes, seed: int = 0) -> int:
    n, i = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = _xround(v[k], int.from_bytes(data[i + 8 * k : i + 8 * k + 8], "little"))
            i += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = ((h ^ _xround(0, v[k])) * _P1 + _P4) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 8 <= n:
        h = (_rotl(h ^ _xround(0, int.from_bytes(data[i : i + 8], "little")), 27) * _P1 + _P4) & _M
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (int.from_bytes(data[i : i + 4], "little") * _P1 & _M), 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h = _rotl(h ^ (data[i] * _P5 & _M), 11) * _P1 & _M
        i += 1
    h ^= h >> 33
    h = h * _P2 & _M
    h ^= h >> 29
    h = h * _P3 & _M
    return h ^ (h >> 32)


# ---- bit streams ----------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """fields go in from the low bits up (little-endian bit order: the first field written is the last one a backward reader meets)"""

    def __init__(self):
        self.chunks, self.acc, self.n = [], 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb) or (nb == 0 and v == 0), (v, nb)
        self.acc |= v << self.n
        self.n += nb
        if self.n >= 512:
            k = self.n >> 3
            self.chunks.append((self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little"))
            self.acc >>= 8 * k
            self.n -= 8 * k

    def done(self, final_bit=True) -> bytes:
        if final_bit:
            self.put(1, 1)
        return b"".join(self.chunks) + self.acc.to_bytes((self.n + 7) >> 3, "little")


def backward_stream(fields, final_bit=True) -> bytes:
    """fields [(value, bits)] in the order the decoder READS them -> the stream (4.1: read from the end, below the final 1 bit)"""
    w = BitWriter()
    for v, nb in reversed(fields):
        w.put(v, nb)
    return w.done(final_bit)


class BackReader:
    def __init__(self, data: bytes):
        if not data or data[-1] == 0:
            raise FormatError("a backward bit-stream ends in a zero byte")
        self.d = data
        self.pos = (len(data) - 1) * 8 + data[-1].bit_length() - 1

    def read(self, nb):
        if nb == 0:
            return 0
        if nb > self.pos:
            raise FormatError("a backward bit-stream ran out of bits")
        self.pos -= nb
        b0 = self.pos >> 3
        return (int.from_bytes(self.d[b0 : b0 + 6], "little") >> (self.pos & 7)) & ((1 << nb) - 1)


class FwdReader:
    def __init__(self, data: bytes):
        self.d, self.bit = data, 0

    def peek(self, nb):
        b0 = self.bit >> 3
        return (int.from_bytes(self.d[b0 : b0 + 4], "little") >> (self.bit & 7)) & ((1 << nb) - 1)


# ---- FSE (4.1) ------------------------------------------------------------------------------------------------------------------------
class FseTable:
    """decoding table of a normalised distribution (4.1.1); .source says which mode described it"""

    def __init__(self, norm, log, source="fse"):
        size = 1 << log
        if sum(abs(c) for c in norm) != size:
            raise FormatError("a normalised count does not fill its table")
        self.log, self.norm, self.source = log, list(norm), source
        sym, high = [0] * size, size - 1
        for s, c in enumerate(norm):
            if c == -1:
                sym[high] = s
                high -= 1
        pos, step, mask = 0, (size >> 1) + (size >> 3) + 3, size - 1
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                sym[pos] = s
                pos = (pos + step) & mask
                while pos > high:
                    pos = (pos + step) & mask
        assert pos == 0
        nxt = [1 if c == -1 else c for c in norm]
        self.sym, self.nb, self.base = sym, [0] * size, [0] * size
        for u in range(size):
            ns = nxt[sym[u]]
            nxt[sym[u]] += 1
            self.nb[u] = log - (ns.bit_length() - 1)
            self.base[u] = (ns << self.nb[u]) - size
        self._owner = {}

    @classmethod
    def rle(cls, symbol):
        t = cls.__new__(cls)
        t.log, t.norm, t.source, t.sym, t.nb, t.base, t._owner = 0, None, "rle", [symbol], [0], [0], {}
        return t

    def symbols(self):
        return set(self.sym)

    def state_for(self, symbol, nxt=None):
        """the state that emits `symbol` and whose interval [base, base + 2^nb) holds the next state (exactly one does); nxt None: the
        sequence is the last one, any state of the symbol will do -- the first"""
        if nxt is None:
            return self.sym.index(symbol)
        own = self._owner.get(symbol)
        if own is None:
            own = [None] * len(self.sym)
            for u, s in enumerate(self.sym):
                if s == symbol:
                    for k in range(self.base[u], self.base[u] + (1 << self.nb[u])):
                        assert own[k] is None
                        own[k] = u
            self._owner[symbol] = own
        return own[nxt]


def default_table(t):
    norm, log = DEFAULTS[t]
    return FseTable(norm, log, "predefined")


def read_ncount(data: bytes, max_sym: int, max_log: int):
    """4.1.1 -> (norm, log, bytes used)"""
    r = FwdReader(data)
    if not data:
        raise FormatError("empty table description")
    log = r.peek(4) + 5
    r.bit = 4
    if log > max_log:
        raise FormatError("accuracy log above the table's maximum")
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    norm, prev0 = [], False
    while remaining > 1 and len(norm) <= max_sym:
        if prev0:
            while True:
                rp = r.peek(2)
                r.bit += 2
                norm += [0] * rp
                if rp != 3:
                    break
            if len(norm) > max_sym:
                raise FormatError("table description: too many symbols")
        maxv = 2 * threshold - 1 - remaining
        lo = r.peek(nbits - 1)
        if lo < maxv:
            v = lo
            r.bit += nbits - 1
        else:
            v = r.peek(nbits)
            if v >= threshold:
                v -= maxv
            r.bit += nbits
        c = v - 1
        remaining -= abs(c)
        norm.append(c)
        prev0 = c == 0
        if remaining < 1:
            raise FormatError("table description: counts exceed the table")
        while remaining < threshold and threshold > 1:
            nbits -= 1
            threshold >>= 1
        if r.bit > 8 * len(data):
            raise FormatError("table description runs past the block")
    if remaining != 1:
        raise FormatError("a normalised count does not fill its table")
    return norm, log, (r.bit + 7) >> 3


def write_ncount(norm, log) -> bytes:
    """4.1.1 (counts that do not add up to the table size are written as they are: a description that does not fill its table)"""
    w = BitWriter()
    w.put(log - 5, 4)
    remaining, threshold, nbits = (1 << log) + 1, 1 << log, log + 1
    norm = list(norm)
    while norm and norm[-1] == 0:
        norm.pop()
    s = 0
    while s < len(norm):
        c = norm[s]
        v, maxv = c + 1, 2 * threshold - 1 - remaining
        if v < maxv:
            w.put(v, nbits - 1)
        elif v < threshold:
            w.put(v, nbits)
        else:
            w.put(v + maxv, nbits)
        remaining -= abs(c)
        s += 1
        while remaining < threshold and threshold > 1:
            nbits -= 1
            threshold >>= 1
        if c == 0:
            run = 0
            while s < len(norm) and norm[s] == 0:
                run += 1
                s += 1
            while run >= 3:
                w.put(3, 2)
                run -= 3
            w.put(run, 2)
        if remaining <= 1:
            break
    return w.done(final_bit=False)


def normalise(hist: dict, log: int):
    """some normalised count (sum 2^log, every used symbol at least 1, two symbols at least) for a histogram {symbol: count}"""
    hist = dict(hist)
    if len(hist) == 1:
        hist[next(iter(hist)) + 1 if next(iter(hist)) == 0 else 0] = 1  # (a table of one symbol is what RLE mode is for)
    size, total = 1 << log, sum(hist.values())
    assert len(hist) <= size
    a = {s: max(1, c * size // total) for s, c in hist.items()}
    order = sorted(hist, key=lambda s: -hist[s])
    while sum(a.values()) > size:
        s = max((s for s in order if a[s] > 1), key=lambda s: a[s])
        a[s] -= 1
    a[order[0]] += size - sum(a.values())
    return [a.get(s, 0) for s in range(max(a) + 1)]


# ---- Huffman (4.2) --------------------------------------------------------------------------------------------------------------------
def huf_codes(weights):
    """weights per symbol (all of them, the last one included) -> {symbol: (code, bits)}, table log (4.2.1: codes by increasing weight,
    then by symbol value)"""
    total = sum(1 << (w - 1) for w in weights if w)
    tlog = total.bit_length() - 1
    assert total == 1 << tlog and tlog <= 11, "the weights are no complete tree of at most 11 bits"
    codes, first = {}, 0
    for w in range(1, tlog + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (first >> (w - 1), tlog + 1 - w)
                first += 1 << (w - 1)
    return codes, tlog


def huf_weights_for(data: bytes, max_bits: int = 11):
    """weights of a Huffman code for the data's histogram (lengths limited by halving the counts until they fit)"""
    import heapq

    hist = Counter(data)
    assert len(hist) >= 2 and max(hist) <= 128, "direct weights describe symbols 0..128, and a tree has two leaves at least"
    while True:
        heap = [(c, s, (s,)) for s, c in hist.items()]
        heapq.heapify(heap)
        length = dict.fromkeys(hist, 0)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                length[s] += 1
            heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
        top = max(length.values())
        if top <= max_bits:
            return [top + 1 - length[s] if s in length else 0 for s in range(max(hist) + 1)]
        hist = Counter({s: (c + 1) // 2 for s, c in hist.items()})


def huf_tree_description(weights) -> bytes:
    """direct representation (4.2.1.1): header byte 127 + number of weights, two weights per byte; the last weight is implied"""
    n = len(weights) - 1
    assert 1 <= n <= 128
    w = list(weights[:n]) + [0]
    return bytes([127 + n]) + bytes(w[i] << 4 | w[i + 1] for i in range(0, n, 2))


def huf_stream(codes, data: bytes) -> bytes:
    return backward_stream([codes[b] for b in data])


# ---- the writer -----------------------------------------------------------------------------------------------------------------------
def raw(data):
    return dict(type="raw", data=bytes(data))


def rle(byte, n):
    return dict(type="rle", byte=byte, n=n)


def lit_raw(data, size_format=None):
    return dict(mode="raw", data=bytes(data), size_format=size_format)


def lit_rle(byte, n, size_format=None):
    return dict(mode="rle", data=bytes([byte]) * n, size_format=size_format)


def lit_huf(data, streams=1, weights=None, size_format=None, **hacks):
    """weights: per symbol, all of them (None: chosen from the data).  hacks: zero_last_byte (of the last stream), extra_bit (one
    more bit in the last stream than its symbols use)"""
    return dict(mode="huf", data=bytes(data), streams=streams, weights=weights, size_format=size_format, **hacks)


def lit_treeless(data, streams=1, size_format=None, **hacks):
    """hacks: force (write it although the frame has no tree yet: with the codes of a two-symbol tree)"""
    return dict(mode="treeless", data=bytes(data), streams=streams, size_format=size_format, **hacks)


def off(distance):
    """the Offset_Value of a new offset"""
    return distance + 3


def compressed(lits, seqs=(), modes=("predefined",) * 3, norms=None, logs=None, count_bytes=None, **hacks):
    """seqs: [(literal length, match length, Offset_Value)] -- Offset_Value 1..3 are the repeat codes, off(d) a new offset.
    modes / norms / logs: per table in the order LL, OF, ML; norms[t] None: computed from the codes used.
    hacks: extra_bit / zero_last_byte (the sequence bit-stream), reserved (the low two bits of the modes byte), ncount_short (table t's
    description with one count lowered by one), log_over (table t's accuracy log one above its maximum), size_delta (added to the
    block header's size)"""
    return dict(type="compressed", lits=lits, seqs=list(seqs), modes=tuple(modes), norms=norms or (None,) * 3, logs=logs or (None,) * 3,
                count_bytes=count_bytes, **hacks)


def frame(blocks, single=True, fcs="auto", window_log=None, checksum=False, **hacks):
    """fcs: bytes of Frame_Content_Size (0 = none, "auto" = the smallest that holds it).  hacks: reserved, dict_id, fcs_delta (added to
    the stated content size), checksum_xor, block_type3 (index of a block whose type becomes 3)"""
    return dict(blocks=list(blocks), single=single, fcs=fcs, window_log=window_log, checksum=checksum, **hacks)


def skippable(payload=b"\x09\x09", nibble=0):
    return dict(skippable=bytes(payload), nibble=nibble)


class _FrameState:
    def __init__(self):
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.tables = [None, None, None]
        self.huf = None  # (codes, weights)
        self.ok = True   # the sequences could be executed


def _literals_section(st: _FrameState, lit) -> bytes:
    data, mode, sf = lit["data"], lit["mode"], lit.get("size_format")
    n = len(data)
    if mode in ("raw", "rle"):
        if sf is None:
            sf = 0 if n < 32 else 1 if n < 4096 else 3
        body = data if mode == "raw" else data[:1]
        t = 0 if mode == "raw" else 1
        if sf in (0, 2):
            assert n < 32
            return bytes([t | sf << 2 | n << 3]) + body
        if sf == 1:
            assert n < 4096
            return (t | 1 << 2 | n << 4).to_bytes(2, "little") + body
        return (t | 3 << 2 | n << 4).to_bytes(3, "little") + body
    tree = b""
    if mode == "huf":
        weights = lit["weights"] or huf_weights_for(data)
        codes, _ = huf_codes(weights)
        st.huf = (codes, list(weights))
        tree = huf_tree_description(weights)
    assert st.huf is not None or lit.get("force"), "treeless literals need a tree (force=True writes them anyway)"
    codes = st.huf[0] if st.huf else huf_codes([1, 1])[0]
    streams = lit["streams"]
    if streams == 1:
        body = huf_stream(codes, data)
        parts = [body]
    else:
        seg = (n + 3) // 4
        parts = [huf_stream(codes, data[k * seg : (k + 1) * seg if k < 3 else n]) for k in range(4)]
    if lit.get("extra_bit"):  # one bit more than the symbols use: the stream is not consumed exactly
        parts[-1] = backward_stream([codes[b] for b in (data if streams == 1 else data[3 * ((n + 3) // 4) :])] + [(0, 1)])
    if lit.get("zero_last_byte"):
        parts[-1] = parts[-1] + b"\x00"
    body = parts[0] if streams == 1 else b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
    csize = len(tree) + len(body)
    if sf is None:
        sf = (0 if streams == 1 else 1) if max(n, csize) < 1024 else 2 if max(n, csize) < 16384 else 3
    assert (sf == 0) == (streams == 1), "size format 0 is the one-stream form, 1..3 have four streams"
    t = 2 if mode == "huf" else 3
    if sf < 2:
        assert n < 1024 and csize < 1024
        h = (t | sf << 2 | n << 4 | csize << 14).to_bytes(3, "little")
    elif sf == 2:
        assert n < 16384 and csize < 16384
        h = (t | sf << 2 | n << 4 | csize << 18).to_bytes(4, "little")
    else:
        assert n < (1 << 18) and csize < (1 << 18)
        h = (t | sf << 2 | n << 4 | csize << 22).to_bytes(5, "little")
    return h + tree + body


def _execute(st: _FrameState, lits: bytes, seqs, frame_start: int):
    """run the sequences on the output so far (3.1.1.4, 3.1.1.5: repeat offsets); an offset that reaches before the frame, or a
    zero offset, or more literals than there are, leaves st.ok False"""
    lp, out = 0, st.out
    for ll, ml, ov in seqs:
        if lp + ll > len(lits):
            st.ok = False
            return
        out += lits[lp : lp + ll]
        lp += ll
        rep = st.rep
        if ov > 3:
            d = ov - 3
            st.rep = [d, rep[0], rep[1]]
        else:
            idx = ov + (1 if ll == 0 else 0)
            if idx == 1:
                d = rep[0]
            elif idx == 2:
                d = rep[1]
                st.rep = [d, rep[0], rep[2]]
            elif idx == 3:
                d = rep[2]
                st.rep = [d, rep[0], rep[1]]
            else:
                d = rep[0] - 1
                st.rep = [d, rep[0], rep[1]]
        if d == 0 or d > len(out) - frame_start:
            st.ok = False
            return
        if d >= ml:
            start = len(out) - d
            out += out[start : start + ml]
        else:
            pat = bytes(out[len(out) - d :])
            out += (pat * (ml // d + 1))[:ml]
    out += lits[lp:]


def _sequences_section(st: _FrameState, blk) -> bytes:
    seqs = blk["seqs"]
    n = len(seqs)
    cb = blk.get("count_bytes")
    if cb is None:
        cb = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if cb == 1:
        assert n < 128
        head = bytes([n])
    elif cb == 2:
        assert n < 0x7F00
        head = bytes([128 + (n >> 8), n & 255])
    else:
        assert n >= 0x7F00
        head = b"\xff" + (n - 0x7F00).to_bytes(2, "little")
    if n == 0:
        return head
    codes = [[], [], []]
    extra = []
    for ll, ml, ov in seqs:
        lc, mc, oc = code_of(LL_BASE, ll), code_of(ML_BASE, ml), ov.bit_length() - 1
        codes[LL].append(lc)
        codes[OF].append(oc)
        codes[ML].append(mc)
        extra.append(((ov - (1 << oc), oc), (ml - ML_BASE[mc], ML_BITS[mc]), (ll - LL_BASE[lc], LL_BITS[lc])))
    modes_byte, desc, tabs = blk.get("reserved", 0), b"", []
    for t in (LL, OF, ML):
        mode = blk["modes"][t]
        modes_byte |= MODES.index(mode) << (6 - 2 * t)
        if mode == "predefined":
            tab = default_table(t)
        elif mode == "rle":
            assert len(set(codes[t])) == 1, "RLE mode: one code for every sequence"
            tab = FseTable.rle(codes[t][0])
            desc += bytes([codes[t][0]])
        elif mode == "fse":
            log = blk["logs"][t] or 6
            norm = blk["norms"][t] or normalise(Counter(codes[t]), log)
            tab = FseTable(norm, log)
            d = write_ncount(norm, log)
            if blk.get("ncount_short") == t:
                # the same bits with the last count lowered by one: the description ends with the table one cell short
                k = max(i for i, c in enumerate(norm) if c > 1)
                short = list(norm)
                short[k] -= 1
                d = write_ncount(short, log)
            if blk.get("log_over") == t:
                d = bytes([(d[0] & 0xF0) | (MAX_LOG[t] + 1 - 5)]) + d[1:]
            desc += d
        else:
            tab = st.tables[t]
            if tab is None:  # Repeat_Mode with nothing to repeat (a near miss): the bit-stream is written for the predefined table
                tab = default_table(t)
        tabs.append(tab)
        if mode != "repeat" or st.tables[t] is not None:
            st.tables[t] = tab
    # 3.1.1.3.2.1.2: the decoder reads the three initial states (LL, OF, ML), then per sequence the offset, match-length and
    # literal-length bits and -- except after the last -- the new LL, ML and OF states.  Going backwards every state is determined.
    states = [[0] * n for _ in range(3)]
    for t in (LL, OF, ML):
        nxt = None
        for i in range(n - 1, -1, -1):
            nxt = states[t][i] = tabs[t].state_for(codes[t][i], nxt)
            assert nxt is not None, "a code is not in its table"
    fields = [(states[t][0], tabs[t].log) for t in (LL, OF, ML)]
    for i in range(n):
        fields += extra[i]
        if i + 1 < n:
            for t in (LL, ML, OF):
                s = states[t][i]
                fields.append((states[t][i + 1] - tabs[t].base[s], tabs[t].nb[s]))
    if blk.get("extra_bit"):
        fields.append((0, 1))
    stream = backward_stream(fields)
    if blk.get("zero_last_byte"):
        stream += b"\x00"
    return head + bytes([modes_byte]) + desc + stream


def _block_header(last, btype, size):
    return (int(last) | btype << 1 | size << 3).to_bytes(3, "little")


def _build_frame(f):
    st = _FrameState()
    body = b""
    nb = len(f["blocks"])
    for i, blk in enumerate(f["blocks"]):
        last = i + 1 == nb and not f.get("no_last")
        if blk["type"] == "raw":
            body += _block_header(last, 0, len(blk["data"])) + blk["data"]
            st.out += blk["data"]
        elif blk["type"] == "rle":
            body += _block_header(last, 1, blk["n"]) + bytes([blk["byte"]])
            st.out += bytes([blk["byte"]]) * blk["n"]
        else:
            content = _literals_section(st, blk["lits"]) + _sequences_section(st, blk)
            body += _block_header(last, 2, len(content) + blk.get("size_delta", 0)) + content
            _execute(st, blk["lits"]["data"], blk["seqs"], 0)
    if f.get("block_type3") is not None:  # the first block's type bits become 3 (Reserved)
        assert f["block_type3"] == 0
        body = bytes([body[0] | 6]) + body[1:]
    content = bytes(st.out)
    stated = len(content) + f.get("fcs_delta", 0)
    fcs, single = f["fcs"], f["single"]
    if fcs == "auto":
        fcs = 1 if stated < 256 and single else 2 if 256 <= stated < 65536 + 256 else 4 if stated < (1 << 32) else 8
    assert fcs in (0, 1, 2, 4, 8) and (fcs != 1 or single) and (fcs != 0 or not single), "no such header form"
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs]
    dict_id = f.get("dict_id")
    fhd = flag << 6 | int(single) << 5 | (8 if f.get("reserved") else 0) | int(f["checksum"]) << 2 | (1 if dict_id is not None else 0)
    head = MAGIC + bytes([fhd])
    if not single:
        head += bytes([((f["window_log"] or 17) - 10) << 3])
    if dict_id is not None:
        head += bytes([dict_id])
    if fcs:
        head += (stated - (256 if fcs == 2 else 0)).to_bytes(fcs, "little")
    tail = b""
    if f["checksum"]:
        tail = ((xxh64(content) & 0xFFFFFFFF) ^ f.get("checksum_xor", 0)).to_bytes(4, "little")
    return head + body + tail, (content if st.ok else None)


def build(spec):
    """spec: a frame(...) or a list of frame(...) and skippable(...) -> (bytes, the bytes it regenerates or None where its own
    sequences cannot be executed).  A frame wrong on purpose still gets the output its sequences describe: the case table says it is
    meant to be rejected."""
    items = spec if isinstance(spec, list) else [spec]
    data, out, ok = b"", b"", True
    for it in items:
        if "skippable" in it:
            data += bytes([0x50 | it["nibble"], 0x2A, 0x4D, 0x18]) + len(it["skippable"]).to_bytes(4, "little") + it["skippable"]
        else:
            d, o = _build_frame(it)
            data += d
            ok = ok and o is not None
            out += o or b""
    return data, (out if ok else None)


# ---- the census -----------------------------------------------------------------------------------------------------------------------
def census(data: bytes, seq_limit: int | None = None) -> Counter:
    """Counts of the format features in a frame or a concatenation of frames (the keys are listed in FEATURES of
    tests/zstd_format_frames.py; the ones an ENCODER's frames are asked for -- literal counts lit_n*, stream starts and ends mod 4 / 32,
    where a Raw_Block stands, accuracy logs -- in REACHABLE of tests/test_zstd_encoder_units_cases.py).  Headers of every frame, block, literals and sequences section are read; the sequence bit-streams
    are decoded (tables built, read backwards) for the codes, the offset forms and the positions.  seq_limit: after that many
    sequences of a frame the remaining blocks' bit-streams are not decoded (counted as seq_blocks_skipped) and the features that
    need positions stop for that frame.  Raises FormatError on what it cannot walk."""
    data = bytes(data)
    c = Counter()
    ip = 0
    nframes = 0
    while ip < len(data):
        if len(data) - ip < 4:
            raise FormatError("truncated magic")
        magic = int.from_bytes(data[ip : ip + 4], "little")
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            size = int.from_bytes(data[ip + 4 : ip + 8], "little")
            if len(data) - ip < 8 + size:
                raise FormatError("truncated skippable frame")
            c["skippable"] += 1
            c["skippable_first" if nframes == 0 and ip == 0 else "skippable_after_frame"] += 1
            ip += 8 + size
            if ip == len(data) and nframes:
                c["skippable_last"] += 1
            continue
        if data[ip : ip + 4] != MAGIC:
            raise FormatError("no frame magic")
        if nframes:
            c["concatenated"] += 1
        nframes += 1
        c["frames"] += 1
        ip = _census_frame(data, ip, c, seq_limit)
    return c


def _census_frame(data, ip, c, seq_limit):
    fhd = data[ip + 4]
    flag, single = fhd >> 6, (fhd >> 5) & 1
    if fhd & 8:
        raise FormatError("reserved bit")
    if fhd & 3:
        raise FormatError("dictionary id")
    p = ip + 5
    if single:
        c["single_segment"] += 1
    else:
        c["window_descriptor"] += 1
        p += 1
    fcs = (1 if single else 0) if flag == 0 else (2, 4, 8)[flag - 1]
    c[f"fcs_{fcs}"] += 1
    content = None
    if fcs:
        content = int.from_bytes(data[p : p + fcs], "little") + (256 if fcs == 2 else 0)
        if content == 0:
            c["content_0"] += 1
        if fcs == 2:
            c[f"fcs_2_content_{content}"] += 1
        if fcs == 1 and content == 255:
            c["fcs_1_content_255"] += 1
    if not single:
        c["window_with_fcs" if fcs else "window_without_fcs"] += 1
    p += fcs
    if fhd & 4:
        c["checksum"] += 1
    # 3.1.1.2: no block is larger than Block_Maximum_Size = min(Window_Size, 128 KiB); a single-segment frame's window is its content
    if single:
        window = content
    else:
        wd = data[ip + 5]
        window = (1 << (10 + (wd >> 3))) + ((1 << (10 + (wd >> 3))) >> 3) * (wd & 7)
    block_max = min(window, BLOCK_MAX)
    # per-frame state
    tables = [None, None, None]
    table_age = [None, None, None]  # what lay between the block that set the table and now: set of "zero_seq", "raw", "rle"
    huf_age = None                  # likewise for the tree: set of "raw_lits", "raw", "rle"; empty: the block before had it
    rep = [(1, "init", -1), (4, "init", -1), (8, "init", -1)]  # (value, "init" or "set", block that set it)
    regions = []  # (start, end, type) of every block's output
    pos, pos_known, nseq_frame, bi, types = 0, True, 0, 0, []
    while True:
        if len(data) - p < 3:
            raise FormatError("truncated block header")
        bh = int.from_bytes(data[p : p + 3], "little")
        last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
        p += 3
        name = ("raw", "rle", "compressed")[btype] if btype < 3 else None
        if name is None:
            raise FormatError("block type 3")
        c[f"block_{name}"] += 1
        if last:
            c[f"last_{name}"] += 1
        if bsize > block_max:
            raise FormatError("block above Block_Maximum_Size")
        start = pos
        c[f"block_start_mod4_{(p - 3 - ip) & 3}"] += 1  # (of the Block_Header, from the frame's first byte)
        if btype == 0 and bsize:
            c["raw_block_first" if bi == 0 else "raw_block_last" if last else "raw_block_mid"] += 1
            if types and types[-1] == "raw":
                c["raw_block_after_raw_block"] += 1
            if any(t is not None for t in tables) or huf_age is not None:
                c["raw_block_after_compressed"] += 1
        if btype == 2 and types and types[-1] == "raw":
            c["compressed_after_raw_block"] += 1
        if btype < 2:
            if btype == 0 and bsize == 0:
                c["raw_block_empty_mid" if not last else "raw_block_empty_last"] += 1
            if btype == 1 and bsize == BLOCK_MAX:
                c["rle_block_131072"] += 1
            p += bsize if btype == 0 else 1
            if p > len(data):
                raise FormatError("truncated block")
            pos += bsize
            for age in table_age:
                if age is not None:
                    age.add(name)
            if huf_age is not None:
                huf_age.add(name)
        else:
            blk = data[p : p + bsize]
            if len(blk) < bsize or bsize < 2:
                raise FormatError("truncated block")
            p += bsize
            # literals section (3.1.1.3.1)
            b0 = blk[0]
            lmode, sf = b0 & 3, (b0 >> 2) & 3
            if lmode < 2:
                lh = 1 if sf in (0, 2) else 2 if sf == 1 else 3
                nlit = int.from_bytes(blk[:lh], "little") >> (3 if lh == 1 else 4)
                csize = nlit if lmode == 0 else 1
                c["lit_raw" if lmode == 0 else "lit_rle"] += 1
                c[f"lit_{'raw' if lmode == 0 else 'rle'}_hdr{lh}"] += 1
                if nlit in (31, 32, 4095, 4096):
                    c[f"lit_{'raw' if lmode == 0 else 'rle'}_n{nlit}"] += 1
                if nlit in LIT_COUNTS:
                    c[f"lit_n{nlit}"] += 1
                if huf_age is not None:
                    huf_age.add("raw_lits")
            else:
                lh = 3 if sf < 2 else 4 if sf == 2 else 5
                h = int.from_bytes(blk[:lh], "little")
                bits = 10 if lh == 3 else 14 if lh == 4 else 18
                nlit, csize = (h >> 4) & ((1 << bits) - 1), h >> (4 + bits)
                streams = 1 if sf == 0 else 4
                c[f"lit_huf_{streams}stream"] += 1
                c[f"lit_huf_hdr{lh}"] += 1
                if nlit in (6, 1023, 1024, 16383, 16384):
                    c[f"lit_huf_{streams}stream_n{nlit}"] += 1
                if nlit in LIT_COUNTS:
                    c[f"lit_n{nlit}"] += 1
                    c[f"lit_huf_n{nlit}"] += 1
                tree = 0
                if lmode == 2:
                    c["lit_huf_tree"] += 1
                    hb = blk[lh]
                    if hb >= 128:
                        nw = hb - 127
                        c["huf_direct"] += 1
                        c["huf_direct_odd" if nw & 1 else "huf_direct_even"] += 1
                        tree = 1 + (nw + 1) // 2
                        w = [(blk[lh + 1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(nw)]
                        total = sum(1 << (x - 1) for x in w if x)
                        tlog = total.bit_length()
                        if nw == 1:
                            c["huf_two_symbols"] += 1
                        c[f"huf_max_bits_{tlog}"] += 1
                    else:
                        c["huf_fse"] += 1
                        tree = 1 + hb
                    huf_age = set()
                else:
                    c["lit_treeless"] += 1
                    if huf_age is None:
                        raise FormatError("treeless literals without a tree")
                    if not huf_age:
                        c["treeless_directly_after_tree"] += 1
                    if "raw_lits" in huf_age:
                        c["treeless_after_raw_literals"] += 1
                    if "raw" in huf_age or "rle" in huf_age:
                        c["treeless_after_raw_rle_block"] += 1
                # stream sizes against the 64-bit threshold of a four-symbols-a-time loop
                body = csize - tree
                if streams == 4:
                    jt = blk[lh + tree : lh + tree + 6]
                    sizes = [int.from_bytes(jt[2 * k : 2 * k + 2], "little") for k in range(3)]
                    sizes.append(body - 6 - sum(sizes))
                    if sizes[3] < 1:
                        raise FormatError("four streams: the sizes do not fit")
                    if nlit < 6:
                        raise FormatError("four streams need six literals")
                    if nlit - 3 * ((nlit + 3) // 4) == 0:
                        c["lit_huf_last_stream_empty"] += 1
                    seg = (nlit + 3) // 4
                    c[f"lit_huf_4stream_seg_mod16_{seg & 15}"] += 1  # (a 16-byte literal quad straddles stream ends unless 0)
                    if nlit - 3 * seg == seg - 3:
                        c["lit_huf_4stream_last_shortest"] += 1  # n = 4 k + 1: the last stream is three literals short
                else:
                    sizes = [body]
                at = lh + tree + (6 if streams == 4 else 0)
                for s in sizes:  # (the streams are not decoded; a zero last byte is seen without)
                    if s < 1 or blk[at + s - 1] == 0:
                        raise FormatError("a literal stream ends in a zero byte")
                    # where the stream starts (byte, from the frame's first byte) and where its end mark stands (bit, likewise)
                    first = p - bsize + at - ip
                    c[f"lit_stream_start_mod4_{first & 3}"] += 1
                    c[f"lit_stream_endbit_mod32_{(8 * (first + s - 1) + blk[at + s - 1].bit_length() - 1) & 31}"] += 1
                    at += s
                c["huf_stream_short"] += sum(1 for s in sizes if s < 8)
                c["huf_stream_long"] += sum(1 for s in sizes if s >= 64)
                if lmode == 3:
                    huf_age.clear()  # (the next treeless block comes directly after a block that used the tree)
            q = lh + csize
            if q >= bsize:
                raise FormatError("literals section fills the block")
            # sequences section (3.1.1.3.2)
            s0 = blk[q]
            if s0 < 128:
                nseq, q, form = s0, q + 1, 1
            elif s0 < 255:
                nseq, q, form = ((s0 - 128) << 8) + blk[q + 1], q + 2, 2
            else:
                nseq, q, form = int.from_bytes(blk[q + 1 : q + 3], "little") + 0x7F00, q + 3, 3
            c[f"nbseq_{form}byte"] += 1
            if nseq in (0, 1, 127, 128, 0x7EFF):
                c[f"nbseq_{nseq}"] += 1
            if nseq in (255, 256, 1023, 1024):
                c[f"nbseq_{nseq}"] += 1
            if nseq == 0 and lmode >= 2:
                c["huf_block_without_sequences"] += 1
            if nseq >= 0x7F00:
                c["nbseq_ge_0x7F00"] += 1
            if nseq == 0:
                if q != bsize:
                    raise FormatError("bytes after a zero sequence count")
                pos += nlit
                for age in table_age:
                    if age is not None:
                        age.add("zero_seq")
            else:
                modes = blk[q]
                q += 1
                if modes & 3:
                    raise FormatError("reserved mode bits")
                for t in (LL, OF, ML):
                    m = (modes >> (6 - 2 * t)) & 3
                    c[f"{NAMES[t]}_{MODES[m]}"] += 1
                    if m == 0:
                        if tables[t] is not None and tables[t].source == "predefined":
                            c["predefined_again"] += 1
                        tables[t] = default_table(t)
                    elif m == 1:
                        if blk[q] > MAX_SYM[t]:
                            raise FormatError("RLE symbol out of range")
                        tables[t] = FseTable.rle(blk[q])
                        q += 1
                    elif m == 2:
                        norm, log, used = read_ncount(blk[q:], MAX_SYM[t], MAX_LOG[t])
                        tables[t] = FseTable(norm, log)
                        q += used
                        c[f"{NAMES[t]}_fse_log_{log}"] += 1
                        if sum(1 for x in norm if x == -1) >= 2:
                            c[f"{NAMES[t]}_fse_several_low_probability"] += 1
                        if sum(1 for x in norm if x == 1) >= 2:
                            c[f"{NAMES[t]}_fse_several_count_1"] += 1
                    else:
                        if tables[t] is None:
                            raise FormatError("Repeat_Mode without a table")
                        c[f"repeat_after_{tables[t].source}"] += 1
                        if not table_age[t]:
                            c["repeat_directly"] += 1
                        if "zero_seq" in table_age[t]:
                            c["repeat_across_zero_seq_block"] += 1
                        if "raw" in table_age[t] or "rle" in table_age[t]:
                            c["repeat_across_raw_rle_block"] += 1
                    table_age[t] = set()
                if q >= bsize:
                    raise FormatError("no sequence bit-stream")
                if blk[bsize - 1]:
                    first = p - bsize + q - ip
                    c[f"seq_stream_start_mod4_{first & 3}"] += 1
                    c[f"seq_stream_endbit_mod32_{(8 * (p - 1 - ip) + blk[bsize - 1].bit_length() - 1) & 31}"] += 1
                if any(s > 23 for s in tables[OF].symbols()):
                    c["of_table_holds_codes_above_23"] += 1
                if seq_limit is not None and nseq_frame >= seq_limit:
                    c["seq_blocks_skipped"] += 1
                    pos_known = False
                else:
                    nseq_frame += nseq
                    pos, rep = _census_sequences(c, blk[q:], nseq, tables, nlit, pos, pos_known, rep, regions, bi, types)
        regions.append((start, pos, name))
        types.append(name if btype < 2 or nseq else "zero_seq")
        bi += 1
        if pos - start > BLOCK_MAX:
            raise FormatError("a block regenerates more than 128 KiB")
        if pos - start == BLOCK_MAX and btype == 2:
            c["compressed_block_131072"] += 1
        if last:
            break
    if content is not None and pos_known and content != pos:
        raise FormatError("content size differs")
    if fhd & 4:
        p += 4
    if p > len(data):
        raise FormatError("truncated checksum")
    return p


def _census_sequences(c, stream, nseq, tables, nlit, pos, pos_known, rep, regions, bi, types):
    r = BackReader(stream)
    tl, to, tm = tables
    sl, so, sm = r.read(tl.log), r.read(to.log), r.read(tm.log)
    used_of = set()
    lit_used = 0
    for i in range(nseq):
        lc, oc, mc = tl.sym[sl], to.sym[so], tm.sym[sm]
        if oc > 31:
            raise FormatError("offset code above 31")
        n1 = oc + ML_BITS[mc] + LL_BITS[lc]
        ov = (1 << oc) + (r.read(oc - 16) << 16 | r.read(16) if oc > 16 else r.read(oc))
        ml = ML_BASE[mc] + r.read(ML_BITS[mc])
        ll = LL_BASE[lc] + r.read(LL_BITS[lc])
        c[f"ll_code_{lc}"] += 1
        c[f"ml_code_{mc}"] += 1
        c[f"of_code_{oc}"] += 1
        used_of.add(oc)
        if i + 1 < nseq:
            n2 = tl.nb[sl] + tm.nb[sm] + to.nb[so]
            sl = tl.base[sl] + r.read(tl.nb[sl])
            sm = tm.base[sm] + r.read(tm.nb[sm])
            so = to.base[so] + r.read(to.nb[so])
            if n1 + n2 > 64:
                c["seq_bits_above_64"] += 1
        if oc == 0:
            c["seq_of_bits_0"] += 1
        if ML_BITS[mc] + LL_BITS[lc] == 0:
            c["seq_ml_ll_bits_0"] += 1
        if ov >= 1 << 24:
            c["offset_value_ge_2p24"] += 1
        # repeat offsets (3.1.1.5)
        if ov > 3:
            d = (ov - 3, "set", bi)
            rep = [d, rep[0], rep[1]]
        else:
            c[f"offset_value_{ov}_{'ll0' if ll == 0 else 'll'}"] += 1
            idx = ov + (1 if ll == 0 else 0)
            if idx == 4:
                c["repeat1_minus_one"] += 1
                src = rep[0]
                d = (src[0] - 1, "set", bi)
                rep = [d, rep[0], rep[1]]
            else:
                src = d = rep[idx - 1]
                if idx == 2:
                    rep = [d, rep[0], rep[2]]
                elif idx == 3:
                    rep = [d, rep[0], rep[1]]
            if src[1] == "init":
                c[f"initial_history_{src[0]}_used"] += 1
                if bi == 0 or all(t != "compressed" for t in types):
                    c["initial_history_in_first_block"] += 1
            elif src[2] < bi:
                between = set(types[src[2] + 1 :])
                c["history_across_compressed"] += 1
                for k in ("zero_seq", "raw", "rle"):
                    if k in between:
                        c[f"history_across_{k}"] += 1
        if d[0] == 0:
            raise FormatError("offset 0")
        lit_used += ll
        if lit_used > nlit:
            raise FormatError("more literals used than the block has")
        if pos_known:
            mpos = pos + ll
            if d[0] > mpos:
                raise FormatError("offset before the frame start")
            if d[0] == mpos:
                c["offset_eq_position"] += 1
            if d[0] < ml:
                c["offset_lt_ml"] += 1
            if d[0] == 1 and ml >= 64:
                c["offset_1_long_match"] += 1
            lo, hi = mpos - d[0], min(mpos, mpos - d[0] + ml)
            for a, b, typ in regions:
                if typ != "compressed" and a < hi and lo < b:
                    c[f"match_reads_{typ}_block"] += 1
        pos += ll + ml
    if r.pos != 0:
        raise FormatError("sequence bit-stream not consumed exactly")
    if any(s > 23 for s in tables[OF].symbols()) and all(s <= 23 for s in used_of):
        c["of_codes_above_23_unused"] += 1
    return pos + (nlit - lit_used), rep
