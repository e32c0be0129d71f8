"""Hand-built LZ4 payloads for every corner of the block format and of the decoders in longtail_amd/csrc/k_lz4_decode.hip, and the near
miss one step outside each corner.  tests/test_lz4_format_cases.py proves every row on the CPU (oracle, reference, census);
tests/test_gpu_lz4_format.py sends the rows through every way the library has of decoding them.

A case: name, family, the sequences (tests/lz4_format.py) or raw payload bytes, `caps`: [(capacity, "valid" | "refused")] -- a verdict
belongs to a (payload, capacity) pair --, `feature`: a predicate on the census that says what the case was built for, `large`: it
belongs on the block-parallel path (a capacity of 128 KiB and more), `roomy`: the verdict does not depend on the capacity as long as
the content fits, so the case may also be offered with a capacity of 2 * PD_UNIT ("small cases on the block-parallel path"),
`ref`: "laxer" where the reference's LZ4_decompress_safe is known to accept what the block format forbids (see below).

The verdicts are the block format's rules as LZ4_decompress_safe's safe loop states them:
    input   a length byte of a literal length lies at or before n - 16, one of a match length at or before n - 5;
            the literals of a sequence with a match end at or before n - 8; the final literals end exactly at n;
    output  the literals of a sequence with a match end at or before cap - 12, its match at or before cap - 5; the content fits;
    offset  1 <= offset <= bytes produced so far.
The reference's fast loop (capacity of 64 and more) and its two-stage shortcut skip the n - 8 / cap - 12 test for a sequence of at
most 14 literals that starts 17 bytes or more before the end, and nothing in the reference tests for offset 0 (it produces zeros):
cases that stand on those spots say ref="laxer", everything else is built so that the reference and the strict rules agree."""
from __future__ import annotations

import functools

from tests import lz4_format as Z

U, T = Z.PD_UNIT, Z.PD_TILE
CASES: list = []
_BY_NAME: dict = {}


def case(name, family, seqs=None, caps=(), feature=None, large=False, roomy=False, ref=None, payload=None):
    assert name not in _BY_NAME, name
    c = dict(name=name, family=family, seqs=seqs, payload=payload, caps=list(caps), feature=feature, large=large, roomy=roomy, ref=ref)
    assert c["caps"] and all(v in ("valid", "refused") for _, v in c["caps"])
    _BY_NAME[name] = c
    CASES.append(c)


@functools.lru_cache(maxsize=None)
def built(name: str):
    """(payload bytes, expected bytes | None where no capacity makes the case valid)"""
    c = _BY_NAME[name]
    seqs = c["seqs"]() if callable(c["seqs"]) else c["seqs"]
    data = c["payload"] if c["payload"] is not None else Z.build(seqs)
    want = Z.model(seqs) if any(v == "valid" for _, v in c["caps"]) else None
    return data, want


def size_of(seqs) -> int:
    return sum(len(s[0]) + (s[2] or 0) for s in seqs)


def pairs():
    """every (case, capacity, verdict)"""
    return [(c, cap, v) for c in CASES for cap, v in c["caps"]]


# ---- what the census has to find (tests/lz4_format.py: census()["loose"], the payload's fields without the rules about its end) -------
def with_match(c):
    return [e for e in c["loose"] if e["off"] is not None]


def last_match(c):
    return with_match(c)[-1]


def lits_end(c, e=None):
    e = e or last_match(c)
    return e["lp"] + e["ll"]


def content(c):
    """bytes the written sequences produce (the final literals included)"""
    return c["loose"][-1]["op"] + c["loose"][-1]["ll"]


def in_end(k, ll=None, mlb=None, below=None):
    """the literals of the last sequence with a match end at n - k (and it has ll literals, mlb match-length bytes, every token below `below`)"""
    return lambda c: (lits_end(c) == c["n"] - k and c["loose_end"] == "final" and (ll is None or last_match(c)["ll"] == ll)
                      and (mlb is None or len(last_match(c)["ml_len_at"]) == mlb) and (below is None or c["loose"][-1]["tok"] < below))


def out_end(lits_at=None, match_at=None):
    """... end at (content - lits_at) in the output / its match ends at (content - match_at): the exact capacity is the content"""
    return lambda c: ((lits_at is None or last_match(c)["op"] + last_match(c)["ll"] == content(c) - lits_at)
                      and (match_at is None or last_match(c)["op"] + last_match(c)["ll"] + last_match(c)["ml"] == content(c) - match_at))


OUT_END = {"literals end at cap-12": out_end(lits_at=12), "literals end at cap-11": out_end(lits_at=11), "match ends at cap-5": out_end(match_at=5),
           "match ends at cap-4": out_end(match_at=4)}


def offset_at(i, off, ml=None, produced=None):
    """sequence i has this offset (and match length, and `produced` bytes of output in front of its match); every other offset is legal"""
    def f(c):
        m = with_match(c)
        i_ = i % len(m)
        return (m[i_]["off"] == off and (ml is None or m[i_]["ml"] == ml) and (produced is None or m[i_]["op"] + m[i_]["ll"] == produced)
                and all(1 <= e["off"] <= e["op"] + e["ll"] for j, e in enumerate(m) if j != i_))
    return f


PRE = (Z.lits(50, 1), 5, 6)  # 56 bytes of output in front of the sequence under test (and a payload of 64 bytes and more with it)
ROOM = 1000                  # a capacity that decides nothing


# ---- end of input: a roomy capacity, only n decides --------------------------------------------------------------------------------
# the sequence under test in three forms, one per inner route: short (batch / fast path), one match-length byte (fast path's
# extension), 15 and more literals (general path).  mlb = its match-length bytes.
FORMS = {"short": (6, 8, 0), "one length byte": (6, 4 + 15 + 40, 1), "long literals": (40, 8, 0)}

for form, (L, ml, mlb) in FORMS.items():
    S = (Z.lits(L, 2), 9, ml)
    # after S's literals: 2 offset bytes, mlb length bytes, the final token, f final literals -> the literals end at n - (3 + mlb + f)
    case(f"in: literals end at n-8, {form}", "end of input", [PRE, S, (Z.lits(5 - mlb, 3), None, None)], [(ROOM, "valid")], roomy=True,
         feature=in_end(8, L, mlb))
    case(f"in: literals end at n-7, {form}", "end of input", [PRE, S, (Z.lits(4 - mlb, 3), None, None)], [(ROOM, "refused")], roomy=True,
         feature=in_end(7, L, mlb))
    case(f"in: no final literals after the match, {form}", "end of input", [PRE, S, (b"", None, None)], [(ROOM, "refused")], roomy=True,
         feature=lambda c, mlb=mlb: c["loose"][-1]["ll"] == 0 and c["loose"][-1]["tok"] == c["n"] - 1 and in_end(3 + mlb)(c))
    ok = [PRE, S, (Z.lits(5, 3), None, None)]
    case(f"in: one byte behind the final literals, {form}", "end of input", payload=Z.build(ok) + b"\x00", caps=[(ROOM, "refused")], roomy=True,
         feature=lambda c: lits_end(c, c["loose"][-1]) == c["n"] - 1 and c["loose"][-1]["ll"] == 5 and c["loose_end"] == "truncated")
    case(f"in: the last final literal cut off, {form}", "end of input", payload=Z.build(ok)[:-1], caps=[(ROOM, "refused")], roomy=True,
         feature=lambda c: lits_end(c, c["loose"][-1]) == c["n"] + 1 and c["loose_end"] == "truncated")
# ... and as the last of a run of short sequences that one window holds: the batch path's own copy of the rules
RUN = [(Z.lits(4, 1), 3, 4)] + [(Z.lits(3, i), 2, 5) for i in range(4)]
case("in: literals end at n-8, in a run of short sequences", "end of input", RUN + [(Z.lits(6, 2), 9, 8), (Z.lits(5, 3), None, None)], [(ROOM, "valid")],
     feature=in_end(8, 6, 0, below=48))
case("in: literals end at n-7, in a run of short sequences", "end of input", RUN + [(Z.lits(6, 2), 9, 8), (Z.lits(4, 3), None, None)], [(ROOM, "refused")],
     feature=in_end(7, 6, 0, below=48))
for form, L in (("short", 6), ("long literals", 40)):
    # two match-length bytes, 3 final literals: the second one at n - 5; three and 2: the third at n - 4 (the literals end at n - 8)
    case(f"in: match length byte at n-5, {form}", "end of input", [PRE, (Z.lits(L, 4), 9, 4 + 15 + 255 + 7), (Z.lits(3, 5), None, None)],
         [(ROOM, "valid")], roomy=True, feature=lambda c: last_match(c)["ml_len_at"][-1] == c["n"] - 5 and in_end(8)(c))
    case(f"in: match length byte at n-4, {form}", "end of input", [PRE, (Z.lits(L, 4), 9, 4 + 15 + 510 + 7), (Z.lits(2, 5), None, None)],
         [(ROOM, "refused")], roomy=True, feature=lambda c: last_match(c)["ml_len_at"][-1] == c["n"] - 4 and in_end(8)(c))
# a sequence of at most 14 literals that starts 17 bytes before the end: the strict rules refuse, the reference's fast loop does not look
case("in: literals end at n-7, 12 literals", "end of input", [PRE, (Z.lits(12, 2), 9, 8), (Z.lits(4, 3), None, None)], [(ROOM, "refused")],
     roomy=True, ref="laxer", feature=lambda c: in_end(7, 12, 0)(c) and last_match(c)["tok"] + 1 == c["n"] - 19)  # (17 bytes and more before the end: the fast loop)
case("in: literal length byte at n-16", "end of input", [PRE, (Z.lits(8, 2), 9, 8), (Z.lits(15, 3), None, None)], [(ROOM, "valid")], roomy=True,
     feature=lambda c: c["loose"][-1]["lit_len_at"] == [c["n"] - 16] and c["loose_end"] == "final")
case("in: literal length byte at n-15", "end of input", payload=Z.build([PRE, (Z.lits(8, 2), 9, 8)]) + b"\xf0\x00" + Z.lits(14, 3),
     caps=[(ROOM, "refused")], roomy=True, feature=lambda c: c["loose"][-1]["lit_len_at"] == [c["n"] - 15] and c["loose_end"] == "truncated")
for f in range(17):
    caps = [(f + 50, "valid"), (f, "valid")] + ([(f - 1, "refused")] if f else [])
    case(f"in: {f} final literals alone", "end of input", [(Z.lits(f, 6), None, None)], caps, feature=lambda c: len(c["tokens"]) == 1)

# ---- end of output: the exact capacity, and one more and one less -----------------------------------------------------------------
for form, (L, _, _) in (("short", FORMS["short"]), ("long literals", FORMS["long literals"])):
    for ml, f, what, at_exact in ((7, 5, "literals end at cap-12", "valid"), (6, 5, "literals end at cap-11", "refused")):
        seqs = [PRE, (Z.lits(L, 2), 9, ml), (Z.lits(f, 3), None, None)]
        n = size_of(seqs)
        case(f"out: {what}, {form}", "end of output", seqs, [(n - 1, "refused"), (n, at_exact), (n + 1, "valid")], feature=OUT_END[what])
    # one match-length byte keeps the input side legal with 4 final literals: the match ends at cap - 4
    seqs = [PRE, (Z.lits(L, 2), 9, 4 + 15 + 3), (Z.lits(4, 3), None, None)]
    n = size_of(seqs)
    case(f"out: match ends at cap-4, {form}", "end of output", seqs, [(n - 1, "refused"), (n, "refused"), (n + 1, "valid")],
         feature=lambda c: OUT_END["match ends at cap-4"](c) and in_end(8)(c))
    seqs = [PRE, (Z.lits(L, 2), 9, 9), (Z.lits(5, 3), None, None)]
    n = size_of(seqs)
    case(f"out: match ends at cap-5, {form}", "end of output", seqs, [(n - 1, "refused"), (n, "valid"), (n + 1, "valid")],
         feature=OUT_END["match ends at cap-5"])
    # 13 final literals: one byte less of capacity leaves the match legal (cap - 12) and only the final literals too long
    seqs = [PRE, (Z.lits(L, 2), 9, 9), (Z.lits(13, 3), None, None)]
    n = size_of(seqs)
    case(f"out: the final literals one byte longer than the capacity, {form}", "end of output", seqs, [(n - 1, "refused"), (n, "valid")],
         feature=lambda c: c["loose"][-1]["ll"] == 13 and out_end(match_at=13)(c))
for ml, f, what, at_exact in ((7, 5, "literals end at cap-12", "valid"), (6, 5, "literals end at cap-11", "refused"), (9, 5, "match ends at cap-5", "valid"),
                              (4 + 15 + 3, 4, "match ends at cap-4", "refused")):
    seqs = RUN + [(Z.lits(6, 2), 9, ml), (Z.lits(f, 3), None, None)]
    n = size_of(seqs)
    case(f"out: {what}, in a run of short sequences", "end of output", seqs, [(n - 1, "refused"), (n, at_exact), (n + 1, "valid")],
         feature=lambda c, what=what: OUT_END[what](c) and in_end(8, below=48)(c))
case("out: payload 00", "end of output", payload=b"\x00", seqs=[(b"", None, None)], caps=[(0, "valid"), (1, "valid")], feature=lambda c: c["n"] == 1 and c["loose_end"] == "final")
# (a token's match nibble means nothing when its literals end the payload: 01 is an empty block for any capacity but 0)
case("out: payload 01", "end of output", payload=b"\x01", seqs=[(b"", None, None)], caps=[(0, "refused"), (10, "valid")], feature=lambda c: c["n"] == 1 and c["loose_end"] == "final")
case("out: payload 00 00", "end of output", payload=b"\x00\x00", caps=[(0, "refused"), (10, "refused")], feature=lambda c: c["n"] == 2 and c["loose_end"] == "truncated")
case("out: empty payload", "end of output", payload=b"", caps=[(0, "refused"), (10, "refused")], feature=lambda c: c["n"] == 0 and c["loose"] == [])

# ---- offsets ------------------------------------------------------------------------------------------------------------------------
OFFSETS = (1, 2, 3, 63, 64, 65, 6399, 6400, 6401, 8191, 8192, 8193, 65535)  # 6400 = RING_SAFE
MATCHES = (4, 18, 19, 64, 65, 273, 274, 2047, 2048, 2049, 20000)
assert Z.RING_SAFE == 6400
for off in OFFSETS:
    for ml in MATCHES:
        # `off` + 37 literals, then three more: the source starts 40 bytes into the output
        seqs = [(Z.lits(off + 37, off), 1, 4), (Z.lits(3, ml), off, ml), (Z.lits(12, 7), None, None)]
        case(f"offset {off}, match {ml}", "offsets", seqs, [(size_of(seqs) + 100, "valid"), (size_of(seqs), "valid")], roomy=True,
             feature=lambda c, off=off, ml=ml: c["matches"][1][1:] == (off, ml))
for ml in MATCHES:
    for off, verdict, ref in ((23, "valid", None), (24, "refused", None), (0, "refused", "laxer")):
        what = {23: "everything so far", 24: "one byte more than there is", 0: "0"}[off]
        case(f"offset {what}, match {ml}", "offsets", [(Z.lits(23, 1), off, ml), (Z.lits(12, 7), None, None)],
             [(ml + 200, verdict)], roomy=True, ref=ref, feature=offset_at(0, off, ml, produced=23))
# a bad offset as the first, a middle and the last token of a run of short sequences: inside a batch
for where in (0, 5, 11):
    for off, ref in ((0, "laxer"), (60000, None)):
        seqs = [(Z.lits(2, i), off if i == where else 1 + i % 2, 4 + i % 3) for i in range(12)] + [(Z.lits(12, 7), None, None)]
        case(f"offset {off} at token {where} of a run of short sequences", "offsets", seqs, [(ROOM, "refused")], roomy=True, ref=ref,
             feature=lambda c, where=where, off=off: offset_at(where, off)(c) and with_match(c)[-1]["tok"] == 55 and c["loose"][-1]["tok"] == 60)
# ... and on the token that ends a batch because its match, longer than 64, is the whole wave's to copy (one length byte: 65 and 273 are
# its shortest and its longest); eleven short sequences in front of it, all of it inside one window
for ml in (65, 273):
    for off, ref in ((0, "laxer"), (60000, None)):
        seqs = [(Z.lits(2, i), 1 + i % 2, 4 + i % 3) for i in range(11)] + [(Z.lits(2, 11), off, ml), (Z.lits(12, 7), None, None)]
        case(f"offset {off} at the wave-copied last token of a run of short sequences, match {ml}", "offsets", seqs, [(ROOM, "refused")], roomy=True, ref=ref,
             feature=lambda c, off=off, ml=ml: offset_at(11, off, ml)(c) and with_match(c)[-1]["tok"] == 55 and with_match(c)[-1]["ml_len_at"] == [60])

# in-lane matches of a batch at the offsets where their source leaves the ring (RING_SAFE; 6554 = DEC_RING - 21 x 78, what a batch may
# overwrite) and at the ring's size
for off in (6399, 6400, 6401, 6553, 6554, 6555, 8190, 8191, 8192, 8193):
    seqs = [(Z.lits(off + 50, off), 1, 4)] + [(Z.lits(2, i), off, 4 + (i * 5) % 15) for i in range(12)] + [(Z.lits(2, 3), off, 40), (Z.lits(12, 7), None, None)]
    case(f"a run of short sequences at offset {off}", "offsets", seqs, [(size_of(seqs), "valid")], roomy=True,
         feature=lambda c, off=off: [m[1] for m in c["matches"][1:]] == [off] * 13)

# the largest batch there is: 15 sequences of four bytes, no literals, matches of 64 copied by their own lanes, all at once.  Token a + 13
# writes the ring slots that token a reads when the offset is 8192 - 13 x 64 + (0 .. 63) = 7360 .. 7423, token a + 14 at 7296 .. 7359:
# RING_SAFE = 6400 keeps such offsets out of the ring with room to spare (the source comes from global memory, the match goes to
# the whole wave); these cases hold that, and would show a bound moved up to where the ring is no longer safe.
for off in (6400, 6401, 7295, 7300, 7359, 7400, 7423, 7424):
    seqs = [(Z.lits(off + 50, off), 1, 4)] + [(b"", off, 64)] * 15 + [(Z.lits(12, 7), None, None)]
    case(f"15 matches of 64 without literals at offset {off}", "offsets", seqs, [(size_of(seqs), "valid")], roomy=True,
         feature=lambda c, off=off: c["matches"][1:] == [(off + 54 + 64 * i, off, 64) for i in range(15)] and c["tokens"][15][0] - c["tokens"][1][0] == 56)

# ---- length encodings ---------------------------------------------------------------------------------------------------------------
for n, what in ((15, "15+0"), (15 + 254, "15+254"), (15 + 255, "15+255+0"), (15 + 255 * 3, "15+255*3+0")):
    k = (n - 15) // 255 + 1
    case(f"literal length {what}", "lengths", [PRE, (Z.lits(n, 8), 11, 6), (Z.lits(12, 7), None, None)], [(n + ROOM, "valid")], roomy=True,
         feature=lambda c, k=k: c["len_bytes"][1] == (k, 0))
    case(f"match length {what}", "lengths", [PRE, (Z.lits(6, 8), 11, 4 + n), (Z.lits(12, 7), None, None)], [(n + ROOM, "valid")], roomy=True,
         feature=lambda c, k=k: c["len_bytes"][1] == (0, k))
# runs of 255: the token of a payload's first sequence stands on lane 0 of the window, so a literal length's run of R bytes ends on lane
# R and its terminator stands on lane R + 1 (R = 62: lane 63, R = 63: lane 0 of the next window); a match length's run behind p
# literals starts on lane p + 3.  2047 and 2048 cross the refill seam of the 2 KiB window (each case at the one source residue its place in
# the call gives it; these are large cases, so the wave-per-block decoder meets them under the serial switch only).
RUNS = (62, 63, 64, 65, 127, 128, 2047, 2048)
for R in RUNS:
    n = 15 + 255 * R + 9
    big = n + 100 >= Z.PAR_MIN_CAP
    seqs = [(Z.lits(n, R), 77, 6), (Z.lits(12, 7), None, None)]
    case(f"literal length with a run of {R} bytes of 255", "lengths", seqs, [(size_of(seqs) + (0 if big else 100), "valid")], large=big, roomy=not big,
         feature=lambda c, R=R: c["len_bytes"][0] == (R + 1, 0) and c["tokens"][0] == (0, 0))
    for p in (1, 2, 3):
        seqs = [(Z.lits(p, R), 1, 4 + n), (Z.lits(12, 7), None, None)]
        case(f"match length with a run of {R} bytes of 255 behind {p} literals", "lengths", seqs, [(size_of(seqs) + (0 if big else 100), "valid")],
             large=big, roomy=not big, feature=lambda c, R=R: c["len_bytes"][0] == (0, R + 1))
for R in range(56, 62):  # behind one literal the terminator stands on lane R + 4: 60 .. 65
    seqs = [(Z.lits(1, R), 1, 4 + 15 + 255 * R + 9), (Z.lits(12, 7), None, None)]
    case(f"match length with a run of {R} bytes of 255 behind 1 literal", "lengths", seqs, [(size_of(seqs) + 100, "valid")], roomy=True,
         feature=lambda c, R=R: c["len_bytes"][0] == (0, R + 1))
case("literal length larger than the capacity", "lengths", [(Z.lits(3000, 1), None, None)], [(100, "refused"), (2999, "refused"), (3000, "valid")],
     feature=lambda c: c["loose"][0]["ll"] == 3000 and c["loose_end"] == "final")
case("literal length larger than the capacity and the payload", "lengths", seqs=[(Z.lits(300, 1), None, None, {"lit_len": 15 + 255 * 40})],
     caps=[(100, "refused"), (100000, "refused")], roomy=True, feature=lambda c: c["loose"][0]["ll"] == 15 + 255 * 40 and c["loose_end"] == "truncated")
case("match length larger than the capacity", "lengths", [(Z.lits(8, 1), 3, 5000), (Z.lits(12, 7), None, None)],
     [(1000, "refused"), (5019, "refused"), (5020, "valid")], feature=lambda c: last_match(c)["ml"] == 5000 and content(c) == 5020)

# ---- window phases ------------------------------------------------------------------------------------------------------------------
for L in range(15):
    seqs = [(Z.lits(4, L), 3, 4)] + [(Z.lits(L, i), 1 + (i * 7) % 8, 4 + i % 12) for i in range(40)] + [(Z.lits(12, 7), None, None)]
    case(f"40 sequences of {L} literals", "window phases", seqs, [(size_of(seqs), "valid")], roomy=True,
         feature=lambda c: len(c["tokens"]) == 42 and all(b == (0, 0) for b in c["len_bytes"]))
for k, pattern in enumerate(((0, 14, 3, 9), (14, 14, 14, 1), (5, 0, 0, 13, 2), (11, 12, 13, 14, 0, 1))):
    # one match-length byte on some of them: a sequence of up to 18 payload bytes
    seqs = [(Z.lits(8, k), 3, 4)] + [(Z.lits(pattern[i % len(pattern)], i), 1 + (i * 5) % 8, (4 + i % 9) if i % 3 else 19 + i) for i in range(60)]
    seqs.append((Z.lits(12, 7), None, None))
    case(f"mixed literal lengths {pattern}", "window phases", seqs, [(size_of(seqs), "valid")], roomy=True, feature=lambda c: len(c["tokens"]) == 62)
# 70 literals leave the window behind: the offset seeds it anew, and the next token stands 2 + (match-length bytes) into it
seqs = [(Z.lits(70, nm), 33, 4 + (15 + 255 * (nm - 1) + 5 if nm else 3)) for nm in (0, 1, 2, 3, 4, 0)] + [(Z.lits(12, 7), None, None)]
case("the window seeded by an offset, 0 to 4 match-length bytes behind it", "window phases", seqs, [(size_of(seqs), "valid")], roomy=True,
     feature=lambda c: [b for _, b in c["len_bytes"][:5]] == [0, 1, 2, 3, 4])
seqs = [(Z.lits(4, 1), 2, 4)] + [(b"", 1 + i % 7, 4 + i % 5) for i in range(30)] + [(Z.lits(12, 7), None, None)]
case("4 literals and 30 sequences of three bytes", "window phases", seqs, [(size_of(seqs), "valid")], roomy=True,
     feature=lambda c: [t for t, _ in c["tokens"][1:31]] == list(range(7, 97, 3)))
case("15 literals first in a window", "window phases", [(Z.lits(15, 1), 4, 6), (Z.lits(15, 2), 9, 5), (Z.lits(12, 7), None, None)], [(ROOM, "valid")],
     roomy=True, feature=lambda c: c["len_bytes"][:2] == [(1, 0), (1, 0)])
for at, third in ((63, 9), (64, 10)):
    # tokens at 0, 17, 34 and 46 / 47 (all below 48: the window seeded at 0 does not slide); 14 literals and the offset put the last
    # one's match-length byte at 63 / 64
    seqs = [(Z.lits(14, 1), 3, 4), (Z.lits(14, 2), 5, 4), (Z.lits(third, 3), 7, 4), (Z.lits(14, 4), 8, 4 + 15 + 20), (Z.lits(12, 7), None, None)]
    case(f"match length byte at window position {at}", "window phases", seqs, [(ROOM, "valid")], roomy=True,
         feature=lambda c, at=at: c["tokens"][3][0] == at - 17 and c["len_bytes"][3] == (0, 1))

# ---- copies -------------------------------------------------------------------------------------------------------------------------
for run in (Z.DIRECT_LITS - 1, Z.DIRECT_LITS, Z.DIRECT_LITS + 1, 100000):
    for start in (0, 5, 2043, 4099):  # the run's first output byte (the window's residue mod 16 comes on top of it)
        head = [(Z.lits(start - 4, 9), 1, 4)] if start else []
        # behind the run: a match from the bulk that went to global memory directly, one from the run's last 8 KiB (the ring)
        seqs = head + [(Z.lits(run, start), 20000, 300), (Z.lits(3, 1), 5000, 100), (Z.lits(12, 7), None, None)]
        case(f"literal run of {run} at output position {start}", "copies", seqs, [(size_of(seqs), "valid")], roomy=True,
             feature=lambda c, run=run, start=start: (start, run) in [(o, l) for _, o, l in c["runs"]])
for off in (1, 7, 8193):
    seqs = [(Z.lits(8200, off), off, 3 * Z.DEC_RING + 5), (Z.lits(12, 7), None, None)]
    case(f"match of 3 x 8192 + 5 at offset {off}", "copies", seqs, [(size_of(seqs), "valid")], roomy=True, feature=offset_at(0, off, 3 * Z.DEC_RING + 5, produced=8200))


# ---- the block-parallel path: a capacity of 2 * PD_UNIT and more, a payload of 64 bytes and more ------------------------------------
def filler(until: int, pos: int, seed: int):
    """sequences of 10 payload bytes (6 literals, a match of 60 with one length byte) from payload position `pos` on; the last one has
    as many literals more as it takes to put the NEXT token exactly at `until`"""
    out = []
    while until - pos >= 19:
        out.append((Z.lits(6, seed + len(out)), 6, 60))
        pos += 10
    out.append((Z.lits(until - pos - 4, seed), 6, 60))
    return out


def seam_case(token_at: int):
    def make():
        seqs = filler(token_at, 0, 1)
        seqs.append((Z.lits(6, 2), 5, 60))  # the token at `token_at`, its offset bytes at +7 and +8
        seqs += filler(3 * T, token_at + 10, 3)
        return seqs + [(Z.lits(12, 7), None, None)]
    return make


def large_case(name, seqs_fn, caps_fn, feature=None, family="block-parallel"):
    seqs = seqs_fn() if callable(seqs_fn) else seqs_fn
    case(name, family, seqs, caps_fn(size_of(seqs)), feature=feature, large=True)


exact = lambda n: [(n, "valid")]  # noqa: E731
for name, at in (("a token at a tile's first byte", T), ("a token at a tile's last byte", T - 1), ("offset bytes split across a tile seam", T - 8)):
    large_case(f"seam: {name}", seam_case(at), exact, feature=lambda c, at=at: at in [t for t, _ in c["tokens"]] and c["size"] >= Z.PAR_MIN_CAP)
large_case("a literal run of 20000 in the middle", [(Z.lits(100, 1), 50, 60), (Z.lits(7, 2), 3, 9), (Z.lits(20000, 3), 30, 50000), (Z.lits(10, 4), 7, 80000),
                                                    (Z.lits(12, 7), None, None)], exact, feature=lambda c: 1 in c["empty_tiles"])
for d in (-1, 0, 1):
    large_case(f"first sequence's literals end at a unit boundary {d:+d}", [(Z.lits(2 * U + d, d + 2), 1000, 1000), (Z.lits(5, 1), 3, 70000), (Z.lits(12, 7), None, None)],
               exact, feature=lambda c, d=d: c["runs"][0][2] == 2 * U + d and len(c["empty_tiles"]) >= 15)
# parallel chains: 00 00 03 is a sequence without literals, a match of 4 at offset 0x0300; read from its second byte it is a match of 4
# at offset 3, from its third a match of 7 at offset 0: three chains that never merge
large_case("parallel chains: 00 00 03 x 30000", [(Z.lits(800, 1), 9, 4)] + [(b"", 0x0300, 4)] * 30000 + [(Z.lits(12, 7), None, None)],
           lambda n: [(Z.PAR_MIN_CAP, "valid")], feature=lambda c: c["size"] == 120816 and c["ntiles"] == 12 and sum(not h for h in c["runin"].values()) >= 4)


def false_chain(fill: bytes):
    def make():
        seqs = filler(T - 600, 0, 5)
        seqs.append((fill, 6, 60))  # 1200 literals around the tile's first byte
        return seqs + filler(3 * T, len(Z.build(seqs)), 6) + [(Z.lits(12, 7), None, None)]
    return make


# how the guess that starts inside the fill ends: 00 (sequences of three bytes) and F0 (255 literals each) run on through the tile beside
# the true chain, FF (one endless length) is invalid at once
for what, fill, ends in (("00", b"\x00" * 1200, "through"), ("FF", b"\xff" * 1200, "invalid"), ("F0", b"\xf0" * 1200, "through")):
    large_case(f"literals that parse as a chain: {what}", false_chain(fill), exact,
               feature=lambda c, ends=ends: (c["runin"][1] is False and c["runin_end"][1] == ends
                                             and any(lp < T - Z.PD_RUNIN and T < lp + ll for lp, _, ll in c["runs"])))
# ... and a false chain that ends like a proper payload: behind 00 00 03 x 8100 the final literals 00 . . 00 . . 50 and five more are,
# read from their first byte, two sequences without literals and a final one of 5 literals.  The walk that starts 512 bytes before
# the fourth tile stands on that phase, and its record says "final".
large_case("literals that parse as a chain: a proper final sequence",
           [(Z.lits(800, 1), 9, 4)] + [(b"", 0x0300, 4)] * 8100 + [(b"\x00ab\x00cd\x50" + Z.lits(5, 2), None, None)], lambda n: [(Z.PAR_MIN_CAP, "valid")],
           feature=lambda c: c["ntiles"] == 4 and c["runin"][3] is False and c["runin_end"][3] == "final")
# units: which of them read below their start is the census's to say (the path-proof test counts them)
large_case("units: a source at a unit's first byte", [(Z.lits(U + 100, 1), 100, 300), (Z.lits(12, 7), None, None)], lambda n: [(2 * U, "valid")],
           feature=lambda c: c["units"] == {})
large_case("units: a source one byte below a unit's first byte", [(Z.lits(U + 100, 1), 101, 300), (Z.lits(12, 7), None, None)], lambda n: [(2 * U, "valid")],
           feature=lambda c: c["units"] == {1: U - 1})
large_case("units: a match across a unit boundary", [(Z.lits(U - 50, 1), 20, 200), (Z.lits(12, 7), None, None)], lambda n: [(2 * U, "valid")],
           feature=lambda c: c["units"] == {1: U - 20})
large_case("units: a match of 140000 from the first unit", [(Z.lits(1000, 1), 1000, 140000), (Z.lits(12, 7), None, None)], exact,
           feature=lambda c: sorted(c["units"]) == [1, 2])
large_case("units: unit 2 reads unit 1, which read unit 0", [(Z.lits(U + 10, 1), 65535, 60000), (Z.lits(5526, 2), 65535, 60000), (Z.lits(12, 7), None, None)], exact,
           feature=lambda c: c["units"] == {1: 11, 2: U + 1})
large_case("units: offset 65535 across a boundary", [(Z.lits(U + 19, 1), 65535, 70000), (Z.lits(12, 7), None, None)], exact,
           feature=lambda c: c["units"] == {1: 20, 2: U + 1})
large_case("units: offset 1 across ten units", [(Z.lits(10, 1), 1, 10 * U + 5), (Z.lits(12, 7), None, None)], exact,
           feature=lambda c: sorted(c["units"]) == list(range(1, 11)))
MIXED = [(Z.lits(300, 1), 100, 5000), (Z.lits(9, 2), 4000, 60000), (Z.lits(30000, 3), 2, 20000), (Z.lits(14, 4), 7, 10000)]
large_case("capacity: content of 2 * PD_UNIT", MIXED + [(Z.lits(2 * U - size_of(MIXED), 5), None, None)],
           lambda n: [(n - 1, "refused"), (n, "valid"), (n + 1, "valid")], feature=lambda c: c["size"] == 2 * U)
large_case("capacity: content of 200000", MIXED + [(Z.lits(200000 - size_of(MIXED), 5), None, None)],
           lambda n: [(n - 1, "refused"), (n, "valid"), (n + 1, "valid"), (4 * U, "valid"), (n + 70000, "valid")], feature=lambda c: c["size"] == 200000)
large_case("capacity: content of 3 * PD_UNIT", MIXED + [(Z.lits(3 * U - size_of(MIXED), 5), None, None)],
           lambda n: [(n, "valid"), (n - 1, "refused")], feature=lambda c: c["size"] == 3 * U)

# the same payload on either side of the dispatch rule: 2 * PD_UNIT - 1 is the wave-per-block decoder's, 2 * PD_UNIT the block-parallel path's
large_case("capacity: content of 100000 around the dispatch rule", MIXED[:2] + [(Z.lits(100000 - size_of(MIXED[:2]), 5), None, None)],
           lambda n: [(2 * U - 1, "valid"), (2 * U, "valid"), (2 * U + 1, "valid")], feature=lambda c: c["size"] == 100000)
MIXED2 = MIXED + [(Z.lits(20, 9), 11, 8000)]
for ml, f, what, at_exact in ((7, 5, "literals end at cap-12", "valid"), (6, 5, "literals end at cap-11", "refused"), (9, 5, "match ends at cap-5", "valid"),
                              (4 + 15 + 3, 4, "match ends at cap-4", "refused")):
    large_case(f"capacity: the last {what}", MIXED2 + [(Z.lits(6, 2), 9, ml), (Z.lits(f, 3), None, None)],
               lambda n, at_exact=at_exact: [(n, at_exact), (n + 1, "valid")], feature=lambda c: c["size"] > 2 * U)

FAMILIES = ("end of input", "end of output", "offsets", "lengths", "window phases", "copies", "block-parallel")
assert {c["family"] for c in CASES} == set(FAMILIES)


def small_on_parallel():
    """Every small case whose payload the dispatch rule sends to the block-parallel path when the capacity is 2 * PD_UNIT, with its verdict
    there: (case, verdict).  A payload that some capacity makes valid is valid with any larger one (every rule about the output is
    "at or before cap - k"); one that no capacity makes valid is refused there too when the case says `roomy`: its verdict does not hang on
    the capacity.  (What is left are payloads below 64 bytes.)"""
    out = []
    for c in CASES:
        if c["large"] or len(built(c["name"])[0]) < Z.PAR_MIN_PAYLOAD:
            continue
        if any(v == "valid" for _, v in c["caps"]):
            out.append((c, "valid"))
        else:
            assert c["roomy"], c["name"]
            out.append((c, "refused"))
    return out
