"""The hand-built LZ4 payloads of tests/lz4_format_payloads.py, proved on the CPU to be what they claim before
tests/test_gpu_lz4_format.py sends them through the GPU decoders.  For every (case, capacity):
  - the verdict the table states is the oracle's (oracle/lz4_oracle.c: the strict rules of LZ4_decompress_safe's safe loop);
  - a valid case decodes, by the oracle, to the bytes the writer's model computed (append the literals, then out[-off] byte by byte);
  - where oracle/_ref is built, the REFERENCE's LZ4_decompress_safe gives the same verdict and bytes.  The one licensed difference is
    the documented polarity of the oracle (it accepts a subset of what the reference accepts on malformed payloads): the cases marked
    ref="laxer" stand on the two spots where the reference does not look -- offset 0, and the n - 8 rule inside its fast loop -- and
    the test holds the reference to accepting them, so that the mark cannot hide anything else;
  - the census finds in the payload the corner the case is named for.
The decoder's constants that the table is built around are read back from k_lz4_decode.hip."""
from pathlib import Path

import numpy as np
import pytest

from tests import lz4_format as Z
from tests import lz4_format_payloads as P
from tests._libs import have_ref, ref as get_ref

ROOT = Path(__file__).resolve().parent.parent
IDS = [c["name"] for c in P.CASES]


def test_constants_are_the_kernels():
    got = Z.source_constants((ROOT / "longtail_amd" / "csrc" / "k_lz4_decode.hip").read_text())
    assert got == Z.EXPECTED_CONSTANTS
    assert Z.RING_SAFE in P.OFFSETS and Z.DEC_RING in P.OFFSETS and Z.DIRECT_LITS == 24576


def test_writer_and_model_on_the_issue_s_example():
    """8 literals, a match of 4, 5 final literals: 17 payload bytes; refused with a capacity of 17 (the literals end past cap - 12),
    accepted with 117"""
    seqs = [(b"abcdefgh", 8, 4), (b"vwxyz", None, None)]
    data = Z.build(seqs)
    assert data == b"\x80abcdefgh\x08\x00\x50vwxyz" and Z.model(seqs) == b"abcdefghabcdvwxyz"
    assert Z.build([(b"x" * 270, 1, 19 + 255), (b"", None, None)]) == b"\xff\xff\x00" + b"x" * 270 + b"\x01\x00\xff\x00\x00"
    assert Z.model([(b"ab", 2, 7), (b"", None, None)]) == b"ababababa" and Z.model([(b"abc", 1, 4)]) == b"abccccc"
    assert Z.build([(b"abc", None, None, {"lit_len": 15 + 255 * 2})]) == b"\xf0\xff\xff\x00abc"  # a length field that says more than there is
    c = Z.census(data)
    assert c["tokens"] == [(0, 0), (11, 12)] and c["end"] == "final" and c["size"] == 17 and c["matches"] == [(8, 8, 4)]


def oracle_verdict(oracle, data: np.ndarray, cap: int):
    n, out = oracle.lz4_decompress(data, cap)
    return ("valid", out.tobytes()) if n >= 0 else ("refused", None)


@pytest.mark.parametrize("case", P.CASES, ids=IDS)
def test_case(case, oracle):
    data, want = P.built(case["name"])
    arr = np.frombuffer(data, np.uint8).copy() if data else np.zeros(0, np.uint8)
    r = get_ref() if have_ref() else None
    for cap, verdict in case["caps"]:
        what = f"'{case['name']}' with capacity {cap}"
        got, out = oracle_verdict(oracle, arr, cap)
        assert got == verdict, f"{what}: the table says {verdict}, the oracle {got}"
        if verdict == "valid":
            assert out == want, f"{what}: the oracle's bytes are not the model's"
            assert cap >= len(want)
        if r is not None:
            err, rout = r.decompress(0, arr, cap)
            if case["ref"] == "laxer":
                assert verdict == "refused" and err == 0, f"{what}: marked as a spot where the reference is laxer, but it refuses too"
            else:
                assert (err == 0) == (verdict == "valid"), f"{what}: the table says {verdict}, the reference returns {err}"
                if verdict == "valid":
                    assert rout.tobytes() == want, f"{what}: the reference's bytes are not the model's"
    c = Z.census(data)  # (lengths and fields only: a refused payload has them too)
    assert case["feature"] is not None and case["feature"](c), "the census does not find what the case is named for"
    if want is not None:
        assert c["end"] == "final" and c["size"] == len(want), "the census does not walk the payload to its end"
        assert case["large"] == any(cap >= Z.PAR_MIN_CAP for cap, _ in case["caps"])
        if case["large"]:
            assert len(data) >= Z.PAR_MIN_PAYLOAD and len(want) <= (1 << 20)


def test_the_table_has_every_family_and_its_near_misses():
    count = {(f, v): 0 for f in P.FAMILIES for v in ("valid", "refused")}
    for c, _, v in P.pairs():
        count[c["family"], v] += 1
    assert all(count[f, v] > 0 for f in P.FAMILIES for v in ("valid", "refused") if (f, v) not in (("window phases", "refused"), ("copies", "refused")))
    laxer = sorted(c["name"] for c in P.CASES if c["ref"] == "laxer")
    # offset 0 with each of the 11 match lengths, at three places of a run, twice on a wave-copied token; the n - 8 rule once
    assert len(laxer) == 11 + 3 + 2 + 1 and all("offset 0" in n or n == "in: literals end at n-7, 12 literals" for n in laxer)
    small = P.small_on_parallel()
    assert len(small) > 150 and {v for _, v in small} == {"valid", "refused"}


def test_window_phases_cover_the_slide():
    """The tokens of the window-phase family stand at every distance from the window's first byte that the decoder's loop can see: a
    sequence that the window holds ends at most 64 bytes in, and whatever is read outside the window seeds it anew, so 0 .. 64 is all
    there is; 40, 47 and 48 (stay, last to stay, first to slide) are among them.  87 and 88, the far end of the slide's range, cannot
    be reached."""
    seen = set()
    for c in P.CASES:
        if c["family"] == "window phases":
            seen |= Z.window_phases(P.built(c["name"])[0])
    assert set(range(65)) <= seen, sorted(set(range(65)) - seen)


def test_parallel_chains_stay_apart():
    """00 00 03 x 30000: 90820 payload bytes for 120816 of output; the three phases never merge, so the walk that starts 512 bytes before
    a tile is the true chain only where 8192 j - 512 happens to stand on its phase"""
    data, want = P.built("parallel chains: 00 00 03 x 30000")
    c = Z.census(data)
    assert (len(data), len(want), c["ntiles"], len(c["runin"])) == (90820, 120816, 12, 11)
    assert sum(not hit for hit in c["runin"].values()) == 7
