"""A writer for LZ4 blocks, the model of what they decode to, and a census of a payload's chain of tokens: the toolkit of the hand-built
payloads in tests/lz4_format_payloads.py.  Pure Python and numpy; nothing here loads a library.

A payload is a list of sequences `(literals, offset | None, match_length | None)`; the last one has no match.  An element may also
be raw `bytes`, written as they are (damage: a model does not exist then).  LZ4 codes a length in exactly one way (the nibble, then
bytes of 255 and one byte below 255), so there is no non-minimal form to force; what a case may force instead is a length field that
says something else than the literals that follow it: a fourth element `{"lit_len": n}` writes n as the literal length.

The numbers the decoders in longtail_amd/csrc/k_lz4_decode.hip are built around are named once, below; source_constants() reads them
back from the kernel source so that a retuned kernel cannot leave the case table beside its boundaries unnoticed."""
from __future__ import annotations

import re

import numpy as np

WINDOW = 64            # payload bytes in the register window, one per lane
SLIDE = 40             # the prefetched window lies this far on
DEC_IN = 2048          # the payload's LDS window, refilled in one go
DEC_FLUSH = 2048       # the ring leaves for global memory in granules of this size
DEC_RING = 8192        # the output ring in LDS
PD_TILE = 8192         # payload bytes per tile of the block-parallel path
RING_SAFE = DEC_RING - 1792  # a batch's in-lane matches read the ring up to this far back
DIRECT_LITS = 3 * DEC_RING   # a literal run of at least this goes payload -> output directly
PD_UNIT = 65536        # output bytes per unit of the block-parallel path
PD_RUNIN = 512         # a tile's walk starts this far in front of it
PAR_MIN_PAYLOAD = 64   # lthip_lz4_decompress_blocks: payload >= this and capacity >= PAR_MIN_CAP -> block-parallel
PAR_MIN_CAP = 2 * PD_UNIT
INT64_CAP = 1 << 30    # a block on the wave-per-block decoder with a capacity (or payload) of this much selects the int64_t kernel

MINMATCH, LASTLITERALS, MFLIMIT = 4, 5, 12


def source_constants(text: str) -> dict:
    """The same numbers as k_lz4_decode.hip states them (constexpr lines, the batch's RING_SAFE, the literal-run threshold, the slide
    and the dispatch condition); a KeyError or a wrong value means the kernel was retuned."""
    def one(pattern):
        m = re.search(pattern, text)
        assert m, f"k_lz4_decode.hip no longer says /{pattern}/"
        return m

    m = one(r"constexpr uint32_t DEC_IN = (\d+)u, DEC_RING = (\d+)u, DEC_FLUSH = (\d+)u;")
    got = dict(DEC_IN=int(m[1]), DEC_RING=int(m[2]), DEC_FLUSH=int(m[3]))
    m = one(r"constexpr uint32_t PD_UNIT = (\d+)u, PD_TILE = (\d+)u, PD_RUNIN = (\d+)u,")
    got.update(PD_UNIT=int(m[1]), PD_TILE=int(m[2]), PD_RUNIN=int(m[3]))
    got["RING_SAFE"] = got["DEC_RING"] - int(one(r"constexpr uint32_t RING_SAFE = DEC_RING - (\d+)u;")[1])
    got["DIRECT_LITS"] = int(one(r"if \(len >= \(I\)\((\d+)u \* DEC_RING\)\)")[1]) * got["DEC_RING"]
    m = one(r"if \(d > (\d+) && d < (\d+)\) // slide")
    got["SLIDE_FROM"], got["SLIDE_TO"] = int(m[1]), int(m[2])
    got["SLIDE"] = int(one(r"w0 \+= (\d+);")[1])
    got["WINDOW"] = int(one(r"if \(p < w0 \|\| p >= w0 \+ (\d+)\)\s+seed\(p\);")[1])
    m = one(r"dst_caps\[b\] >= (\d+)u \* PD_UNIT && dst_caps\[b\] <= 0x7E000000u && src_sizes\[b\] >= (\d+)u\)")
    got["PAR_MIN_CAP"], got["PAR_MIN_PAYLOAD"] = int(m[1]) * got["PD_UNIT"], int(m[2])
    m = one(r"small = small && src_sizes\[b\] < \(1u << (\d+)\) && dst_caps\[b\] < \(1u << (\d+)\);")
    assert m[1] == m[2]
    got["INT64_CAP"] = 1 << int(m[1])
    return got


EXPECTED_CONSTANTS = dict(DEC_IN=DEC_IN, DEC_RING=DEC_RING, DEC_FLUSH=DEC_FLUSH, PD_UNIT=PD_UNIT, PD_TILE=PD_TILE, PD_RUNIN=PD_RUNIN,
                          RING_SAFE=RING_SAFE, DIRECT_LITS=DIRECT_LITS, SLIDE_FROM=SLIDE + 7, SLIDE_TO=SLIDE + 48, SLIDE=SLIDE, WINDOW=WINDOW,
                          PAR_MIN_CAP=PAR_MIN_CAP, PAR_MIN_PAYLOAD=PAR_MIN_PAYLOAD, INT64_CAP=INT64_CAP)


# ---- the writer -------------------------------------------------------------------------------------------------------------------

def lits(n: int, seed: int = 0) -> bytes:
    """n literal bytes that depend on their position and the seed (no period that a wrong offset would hit again)"""
    i = np.arange(n, dtype=np.uint32) + np.uint32(seed * 7919 + 1)
    return (((i * np.uint32(2246822519)) >> np.uint32(13)) ^ (i >> np.uint32(3))).astype(np.uint8).tobytes()


def length_bytes(rest: int) -> bytes:
    """what follows a nibble of 15: rest = length - 15"""
    assert rest >= 0
    return b"\xff" * (rest // 255) + bytes([rest % 255])


def build(seqs) -> bytes:
    out = bytearray()
    for s in seqs:
        if isinstance(s, (bytes, bytearray)):
            out += s
            continue
        lit, off, ml = s[0], s[1], s[2]
        ll = s[3]["lit_len"] if len(s) > 3 else len(lit)
        assert (off is None) == (ml is None) and (ml is None or ml >= MINMATCH) and (off is None or 0 <= off <= 65535)
        m = 0 if ml is None else ml - MINMATCH
        out.append((min(ll, 15) << 4) | min(m, 15))
        if ll >= 15:
            out += length_bytes(ll - 15)
        out += lit
        if ml is not None:
            out += bytes([off & 255, off >> 8])
            if m >= 15:
                out += length_bytes(m - 15)
    return bytes(out)


def model(seqs) -> bytes:
    """What the sequences produce: the literals, then out[-off] byte by byte (a match longer than its offset repeats its seed).  The
    expected bytes of every valid case come from here and from nowhere else."""
    out = bytearray()
    for s in seqs:
        assert not isinstance(s, (bytes, bytearray)) and len(s) == 3, "no model for a damaged payload"
        lit, off, ml = s
        out += lit
        if ml is not None:
            assert 1 <= off <= len(out), "the offset reaches below the output's start"
            seed = bytes(out[len(out) - off:])
            out += seed[:ml] if ml <= off else (seed * (ml // off + 1))[:ml]  # == byte by byte: byte j of the match is seed[j % off]
    return bytes(out)


# ---- the census ---------------------------------------------------------------------------------------------------------------------

def hop(p: bytes, ip: int):
    """One sequence at ip, lengths only.  -> (kind, next token, literal position, literal length, offset, match length, literal-length
    bytes, match-length bytes); kind 0: a sequence with a match, 1: the final one, 2: nothing that parses"""
    n = len(p)
    if ip >= n:
        return 2, n, 0, 0, 0, 0, 0, 0
    tok = p[ip]
    q = ip + 1
    ll, nl = tok >> 4, 0
    if ll == 15:
        while True:
            if q >= n:
                return 2, n, 0, 0, 0, 0, 0, 0
            v = p[q]
            q += 1
            nl += 1
            ll += v
            if v != 255:
                break
    lp = q
    if q + ll > n - (2 + 1 + LASTLITERALS):
        return (1 if q + ll == n else 2), n, lp, ll, 0, 0, nl, 0
    q += ll
    off = p[q] | (p[q + 1] << 8)
    q += 2
    ml, nm = tok & 15, 0
    if ml == 15:
        while True:
            if q >= n:
                return 2, n, 0, 0, 0, 0, 0, 0
            v = p[q]
            q += 1
            nm += 1
            ml += v
            if v != 255:
                break
    return 0, q, lp, ll, off, ml + MINMATCH, nl, nm


def loose(p: bytes):
    """The fields of the payload as they are written, from position 0, WITHOUT the rules about the block's end (a sequence has a match
    whenever bytes follow its literals): what a near miss consists of even though no decoder accepts it.  -> ([dict(tok, lp, ll, op,
    lit_len_at: positions of the literal length's bytes, off, ml, ml_len_at: positions of the match length's bytes)], how it ends:
    "final" (the last literals end exactly at n) or "truncated" (a field or the literals want bytes past n))"""
    n, ip, op, out = len(p), 0, 0, []
    while ip < n:
        tok, q = p[ip], ip + 1
        e = dict(tok=ip, op=op, off=None, ml=None, lit_len_at=[], ml_len_at=[])
        out.append(e)
        ll = tok >> 4
        if ll == 15:
            while True:
                if q >= n:
                    return out, "truncated"
                e["lit_len_at"].append(q)
                ll += p[q]
                q += 1
                if p[q - 1] != 255:
                    break
        e["lp"], e["ll"] = q, ll
        if q + ll >= n:
            return out, ("final" if q + ll == n else "truncated")
        q += ll
        op += ll
        if q + 2 > n:
            return out, "truncated"
        e["off"] = p[q] | (p[q + 1] << 8)
        q += 2
        ml = tok & 15
        if ml == 15:
            while True:
                if q >= n:
                    return out, "truncated"
                e["ml_len_at"].append(q)
                ml += p[q]
                q += 1
                if p[q - 1] != 255:
                    break
        e["ml"] = ml + MINMATCH
        op += e["ml"]
        ip = q
    return out, "truncated"  # (no final sequence at all: the payload ends behind a match, or is empty)


def census(payload: bytes) -> dict:
    """A length-only walk of the true chain (from position 0), and of the guesses the block-parallel path makes."""
    n = len(payload)
    tokens, len_bytes, matches, runs = [], [], [], []
    ip = op = 0
    end = "damaged"
    while ip < n:
        kind, nxt, lp, ll, off, ml, nl, nm = hop(payload, ip)
        if kind == 2:
            break
        tokens.append((ip, op))
        len_bytes.append((nl, nm))
        runs.append((lp, op, ll))
        op += ll
        if kind == 1:
            end = "final"
            break
        matches.append((op, off, ml))
        op += ml
        ip = nxt
    ntiles = (n + PD_TILE - 1) // PD_TILE
    tok_pos = [t for t, _ in tokens]
    held = {t // PD_TILE for t in tok_pos}
    runin, runin_end = {}, {}
    for j in range(1, ntiles):
        t0 = j * PD_TILE
        true_entry = next((t for t in tok_pos if t >= t0), None)
        if true_entry is None or true_entry >= t0 + PD_TILE:
            continue  # the chain jumps over the tile (or ends before it): nothing to guess
        q = t0 - PD_RUNIN
        while q < t0:
            kind, nxt = hop(payload, q)[:2]
            if kind != 0:
                q = -1
                break
            q = nxt
        runin[j] = q == true_entry
        kind = 0
        while kind == 0 and 0 <= q < t0 + PD_TILE:  # how the guess's walk through the tile ends
            kind, q = hop(payload, q)[:2]
        runin_end[j] = ("through", "final", "invalid")[2 if q < 0 else kind]
    units = {}
    for start, off, ml in matches:
        for k in range(max(1, start // PD_UNIT), (start + ml - 1) // PD_UNIT + 1):
            lo = k * PD_UNIT
            src = max(start, lo) - off
            if src < lo:
                units[k] = min(units.get(k, src), src)
    fields, fields_end = loose(payload)
    return dict(n=n, loose=fields, loose_end=fields_end, tokens=tokens, len_bytes=len_bytes, matches=matches, runs=runs, end=end, size=op, ntiles=ntiles,
                empty_tiles=[j for j in range(ntiles) if j not in held], runin=runin, runin_end=runin_end, units=units)


def window_phases(payload: bytes) -> set:
    """Where the tokens of the true chain stand relative to the register window's first byte when the wave-per-block decoder takes one
    sequence per step (lz4_decode_one, top of its loop, before the slide): the window is seeded at a token, slides by SLIDE when the
    token stands SLIDE + 8 .. SLIDE + 47 bytes in, and is seeded again wherever a byte outside it is read (length bytes, the offset
    after a literal run the general path copied).
    This is a restatement in Python of lz4_decode_one's windowing, read off k_lz4_decode.hip; only its numbers (the window's size, the
    slide and its range) are tied to the source (source_constants), the logic is not checked against the kernel by anything."""
    n = len(payload)
    seen, ip, w0 = set(), 0, -1000
    while ip < n:
        d = ip - w0
        if 0 <= d < 200:
            seen.add(d)
        if SLIDE + 7 < d < SLIDE + 48:
            w0 += SLIDE
            d -= SLIDE
        if d < 0 or d > SLIDE + 7:
            w0, d = ip, 0
        seen.add(d)
        kind, nxt, lp, ll, off, ml, nl, nm = hop(payload, ip)
        if kind != 0:
            break
        e = d + 3 + ll
        if not (ll < 15 and (nm == 0 or (nm == 1 and e <= 63))):
            for q in list(range(ip + 1, ip + 1 + nl)) + list(range(lp + ll, nxt)):  # the general path's reads, in order
                if q < w0 or q >= w0 + WINDOW:
                    w0 = q
        ip = nxt
    return seen


# ---- what an encoder owes -------------------------------------------------------------------------------------------------------------

def lz4_len_bytes(length: int) -> int:
    """the bytes that follow a nibble for this length (k_lz4.hip's lz4_len_bytes): none below 15, then one per 255 and the rest"""
    return (length - 15) // 255 + 1 if length >= 15 else 0


def encoder_rules(payload: bytes, raw_len: int):
    """The fields of the payload (loose()) and the list of what it does against the rules an LZ4 ENCODER has to keep (the block format's
    "end of block restrictions", lz4.c:242-246) -- rules no decoder checks in full: the walk ends "final" at raw_len; 1 <= offset <=
    min(output position, 65535); every match starts at or before raw_len - MFLIMIT and ends at or before raw_len - LASTLITERALS; after
    a match the final literals are LASTLITERALS and more; a source below MFLIMIT + 1 bytes is one literal run; a length has exactly the
    length bytes its value asks for.  -> (fields, [violation, ...]); an empty list is a block every LZ4 decoder has to take."""
    fields, end = loose(payload)
    bad = []
    if end != "final":
        bad.append(f"the walk ends '{end}', not with a final literal run")
    matches = 0
    for k, e in enumerate(fields):
        if "ll" not in e:
            continue  # (truncated inside the literal length: reported above)
        if len(e["lit_len_at"]) != lz4_len_bytes(e["ll"]):
            bad.append(f"sequence {k}: a literal length of {e['ll']} in {len(e['lit_len_at'])} length bytes")
        if e["off"] is None:
            continue
        matches += 1
        start = e["op"] + e["ll"]
        if e["ml"] is None:
            bad.append(f"sequence {k}: the match length is cut off")
            continue
        if len(e["ml_len_at"]) != lz4_len_bytes(e["ml"] - MINMATCH):
            bad.append(f"sequence {k}: a match length of {e['ml']} in {len(e['ml_len_at'])} length bytes")
        if not 1 <= e["off"] <= min(start, 65535):
            bad.append(f"sequence {k}: offset {e['off']} at output position {start}")
        if start > raw_len - MFLIMIT:
            bad.append(f"sequence {k}: a match starts at {start}, {raw_len - start} bytes before the end (at least {MFLIMIT})")
        if start + e["ml"] > raw_len - LASTLITERALS:
            bad.append(f"sequence {k}: a match ends at {start + e['ml']}, {raw_len - start - e['ml']} bytes before the end (at least {LASTLITERALS})")
    if end == "final":
        last = fields[-1]
        if last["op"] + last["ll"] != raw_len:
            bad.append(f"the payload describes {last['op'] + last['ll']} bytes, the source has {raw_len}")
        if matches and last["ll"] < LASTLITERALS:
            bad.append(f"{last['ll']} final literals after a match (at least {LASTLITERALS})")
    if raw_len < MFLIMIT + 1 and matches:
        bad.append(f"a source of {raw_len} bytes with a match (below {MFLIMIT + 1} bytes it is one literal run)")
    return fields, bad
