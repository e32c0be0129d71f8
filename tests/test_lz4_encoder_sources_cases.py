"""The hand-built sources of tests/lz4_encoder_sources.py and the rule checker Z.encoder_rules (tests/lz4_format.py), proved on the CPU
before tests/test_gpu_lz4_encoder_sources.py sends the sources through the GPU encoders:
  - every source compresses with the oracle (bit-exact with LZ4_compress_fast), the payload decodes back with the oracle and, where
    oracle/_ref is built, with the reference, and encoder_rules finds nothing in it;
  - encoder_rules flags hand-written payloads that break one rule each, and accepts the nearest valid neighbour of each;
  - the coverage conditions the GPU test holds the GPU's payloads to hold for the oracle's: a later failure there is the GPU encoder's,
    not the table's;
  - every source's corner is really in it (noise without a 4-byte repeat within reach, the one repeat exactly G back, ...);
  - the numbers the table is built around are the kernel's."""
import functools
from pathlib import Path

import numpy as np
import pytest

from tests import lz4_encoder_sources as S
from tests import lz4_format as Z
from tests._libs import have_ref, ref as get_ref

ROOT = Path(__file__).resolve().parent.parent


def test_constants_are_the_kernels():
    assert S.source_constants(ROOT / "longtail_amd" / "csrc") == S.EXPECTED_CONSTANTS
    assert (S.U, S.H, S.G) == (1 << S.SEGMENT_LOG2, S.G_BATCH << S.SEGMENT_LOG2, S.G_LANES << S.SEGMENT_LOG2) and S.G == S.REACH + 1
    assert S.LANE_EXT == 4 + 16 + 16 and S.U == 64 * S.SUB


@functools.lru_cache(maxsize=None)
def oracle_payloads():
    from tests._libs import oracle

    o = oracle()
    return tuple(o.lz4_compress(s.data) for s in S.sources())


def test_every_source_compresses_round_trips_and_keeps_the_rules(oracle):
    r = get_ref() if have_ref() else None
    srcs = S.sources()
    assert len(srcs) > 1000 and {s.family for s in srcs} == set(S.FAMILIES)
    for s, p in zip(srcs, oracle_payloads()):
        n, out = oracle.lz4_decompress(p, len(s.data))
        assert n == len(s.data) and (out == s.data).all(), s.name
        if r is not None:
            err, out2 = r.decompress(0, p, len(s.data))
            assert err == 0 and len(out2) == len(s.data) and (out2 == s.data).all(), s.name
        fields, bad = Z.encoder_rules(p.tobytes(), len(s.data))
        assert bad == [], f"'{s.name}': {bad}"


# ---- the checker -----------------------------------------------------------------------------------------------------------------------

L = Z.lits
# (what is wrong, a payload that breaks exactly that rule, its source length, the nearest payload that keeps it, its source length)
BROKEN = [
    ("4 final literals after a match", [(L(20, 1), 8, 8), (L(4, 2), None, None)], 32, [(L(20, 1), 8, 8), (L(5, 2), None, None)], 33),
    ("a match starts at n - 11", [(L(20, 1), 8, 6), (L(5, 2), None, None)], 31, [(L(20, 1), 8, 7), (L(5, 2), None, None)], 32),
    ("a match ends at n - 4", [(L(8, 1), 8, 8), (L(4, 2), None, None)], 20, [(L(8, 1), 8, 8), (L(5, 2), None, None)], 21),
    ("offset 0", [(L(20, 1), 0, 8), (L(12, 2), None, None)], 40, [(L(20, 1), 1, 8), (L(12, 2), None, None)], 40),
    ("an offset one beyond the output position", [(L(20, 1), 21, 8), (L(12, 2), None, None)], 40, [(L(20, 1), 20, 8), (L(12, 2), None, None)], 40),
    ("a 12-byte source with a match", [(L(1, 1), 1, 4), (L(7, 2), None, None)], 12, [(L(1, 1), 1, 4), (L(8, 2), None, None)], 13),
]


@pytest.mark.parametrize("what,broken,n,valid,n_valid", BROKEN, ids=[b[0] for b in BROKEN])
def test_encoder_rules_flags_one_step_outside_and_accepts_one_step_inside(what, broken, n, valid, n_valid):
    fields, bad = Z.encoder_rules(Z.build(broken), n)
    assert bad, f"'{what}' passes the checker"
    assert sum(len(s[0]) + (s[2] or 0) for s in broken) == n
    fields, ok = Z.encoder_rules(Z.build(valid), n_valid)
    assert ok == [] and len(Z.model(valid)) == n_valid, (what, ok)
    assert len(fields) == len(valid)


def test_encoder_rules_on_what_is_not_a_block_of_the_source():
    good = Z.build([(L(20, 1), 8, 8), (L(5, 2), None, None)])
    assert Z.encoder_rules(good, 33)[1] == []
    assert Z.encoder_rules(good, 34)[1] and Z.encoder_rules(good, 32)[1]          # another source length
    assert Z.encoder_rules(good[:-1], 32)[1] and Z.encoder_rules(b"", 0)[1]        # truncated; no token at all
    assert Z.encoder_rules(good + b"\x00", 33)[1]                                   # a byte behind the final literals
    assert Z.encoder_rules(b"\x00", 0)[1] == [] and Z.encoder_rules(Z.build([(L(12, 3), None, None)]), 12)[1] == []
    # a length has one coding: 15 literals are the nibble and a zero byte
    assert [Z.lz4_len_bytes(v) for v in (0, 14, 15, 269, 270, 524, 525)] == [0, 0, 1, 1, 2, 2, 3]
    fields, bad = Z.encoder_rules(Z.build([(L(270, 1), 8, 19 + 255), (L(5, 2), None, None)]), 270 + 274 + 5)
    assert bad == [] and len(fields[0]["lit_len_at"]) == 2 and len(fields[0]["ml_len_at"]) == 2


# ---- coverage: what the union of the payloads' fields has to hold ----------------------------------------------------------------------

def test_coverage_conditions_hold_for_the_oracle():
    srcs = S.sources()
    cov = S.Coverage()
    for s, p in zip(srcs, oracle_payloads()):
        cov.add(s, Z.loose(p.tobytes())[0])
    assert cov.missing() == [], cov.missing()
    # what the issue's trial on the CPU saw, over and above the conditions
    assert {14, 15, 16, 269, 270, 271, 524, 525, 526} <= cov.lit_lens and {18, 19, 20, 273, 274, 275, 528, 529, 530} <= cov.match_lens
    assert {1, 2, 3, 4, 5, 7, 8, 65535} <= cov.offsets


# ---- the corners are in the sources ------------------------------------------------------------------------------------------------------

def repeats_in(a, lo, hi):
    r = S.gram_repeats(a)
    return r[(r >= lo) & (r < hi)]


def test_noise_has_no_repeat_within_reach():
    n = S.noise(300000, 5)
    assert S.gram_repeats(n).size == 0
    planted = n.copy()
    planted[200000:200004] = planted[200000 - 65535 : 200000 - 65531]
    assert 200000 in S.gram_repeats(planted)
    planted = n.copy()
    planted[200000:200004] = planted[200000 - 65536 : 200000 - 65532]
    assert 200000 not in S.gram_repeats(planted)  # (one byte out of reach)
    for name in ("stitch steps: 130 units of noise", "nothing repeats: noise(G) | noise'(G)"):
        assert S.gram_repeats(S.by_name(name).data).size == 0, name
    for name, data in S.batch_blocks():
        if name.startswith("no match"):
            assert S.gram_repeats(data).size == 0


def test_the_sources_hold_their_corners():
    a = S.by_name(f"the only repeat lies {S.G} back").data
    assert S.gram_repeats(a).size == 0 and S.gram_repeats(a, reach=S.G).size == 97  # (100 bytes: 97 positions of four)
    a = S.by_name(f"the only repeat lies {S.G - 1} back").data
    r = S.gram_repeats(a)
    assert r.size == 97 and r[0] == S.G - 1 + 300 and S.gram_repeats(a, reach=S.G - 2).size == 0
    for d in S.FAR_IN_GROUP:
        a = S.by_name(f"offset {d} inside one group").data
        far = [p for p in S.gram_repeats(a) if p >= S.H + S.U]
        assert len(far) == 61 and far[0] == 128 + d and 128 + d + 64 <= S.G - 12
    a = S.by_name("stitch steps: 70 units, a match in unit 0, units 1 .. 66 noise, units 67 .. 69 repeat unit 0").data
    assert len(a) == 70 * S.U and repeats_in(a, S.U, 67 * S.U).size == 0 and repeats_in(a, 0, S.U).size and repeats_in(a, 67 * S.U, 70 * S.U).size
    assert (a[67 * S.U : 68 * S.U] == a[: S.U]).all() and (a[69 * S.U :] == a[: S.U]).all()
    for u in (63, 64):
        a = S.by_name(f"stitch steps: 66 units, matches in units 0 and {u} only").data
        r = S.gram_repeats(a)
        assert {int(p) // S.U for p in r} == {0, u}
    a = S.by_name("stitch steps: 70 units, a match in the last unit only").data
    assert {int(p) // S.U for p in S.gram_repeats(a)} == {69}
    # a beacon unit repeats 32 bytes where the classification pass probes them: inside its first 640 bytes, 64 back
    b = S.beacon_unit(1)
    r = S.gram_repeats(b)
    assert list(r) == list(range(S.SUB, S.SUB + 29)) and (b[S.SUB : S.SUB + 32] == b[:32]).all()


def test_the_named_lengths_are_in_the_oracle_s_payloads():
    """a source named for a literal run or a match of a length has a field of that length in the greedy parse"""
    pay = dict(zip((s.name for s in S.sources()), oracle_payloads()))

    def lens(name):
        f = Z.loose(pay[name].tobytes())[0]
        return {e["ll"] for e in f[:-1]}, {e["ml"] for e in f if e["ml"] is not None}

    def repeats(name):
        """the source's repeated stretches [(first byte, length)] and the gaps between them, from the bytes alone: what any parser that
        takes every repeat at its first byte makes of the source (the greedy parse steps ever wider through noise and may miss a
        repeat behind a long run; the GPU's lane parser probes every aligned dword)"""
        r = S.gram_repeats(S.by_name(name).data)
        cut = np.flatnonzero(np.diff(r) != 1)
        first, last = r[np.r_[0, cut + 1]], r[np.r_[cut, len(r) - 1]]
        stretches = [(int(a), int(b) + 4 - int(a)) for a, b in zip(first, last)]
        return stretches, {b[0] - (a[0] + a[1]) for a, b in zip(stretches, stretches[1:])}

    for n in S.LIT_RUNS:
        for name in [f"literal run: A | A[:32] | noise({n}) | A[:40] | noise(9)"] + ([f"literal run: the same with {n} literals, distance % 4 == 0"] if n % 4 else []):
            st, gaps = repeats(name)
            assert st == [(64, 32), (96 + n, 40)] and gaps == {n}, (name, st)
            assert n > 600 or n in lens(name)[0], name
    for total in S.SEAM_SUMS:
        for carry in S.SEAM_CARRIES:
            if carry <= total:
                name = f"literal run: {total} literals over a unit seam, {carry} + {total - carry}"
                st, gaps = repeats(name)
                assert st[1:] == [(S.U - carry - 32, 32), (S.U + total - carry, 40)] and total in lens(name)[0], (name, st)
    through = [s.name for s in S.sources() if "match-less units" in s.name]
    assert len(through) >= 3 * 3 * 2
    for name in through:
        total = int(name.split()[2])
        st, gaps = repeats(name)
        assert len(st) == 3 and st[2][0] - (st[1][0] + 32) == total and st[1][0] + 32 < S.U and st[2][0] % S.U <= 255, (name, st)
        assert (total - 15) % 255 in (0, 1, 254), name  # (at a length byte's boundary, or one beside it)
    for m in S.MATCH_LENGTHS:
        name = f"match length: A(600) | noise(20) | A[:{m}] | noise(30)"
        assert repeats(name)[0] == [(620, m)], name
        assert m < 17 or m in lens(name)[1], m  # (the greedy parse stands at 620 with a step of 4: a match of 4 or 5 it may pass by)
    for s in S.sources():
        if s.family == "match length" and "bytes" in s.name and "beacon" not in s.name:
            m = int(s.name.split()[2])
            st = repeats(s.name)[0]
            assert st[0] == (S.SUB, 32) and st[1][1] == m and len(st) == 2, (s.name, st)


def test_the_batch_lists():
    blocks, lists = S.batch_blocks(), S.batches()
    assert [len(d) for _, d in blocks][:4] == [0, 1, 12, 13] and len(blocks[-1][1]) == 70 * S.U
    n = len(blocks)
    assert lists["reversed"] == lists["as listed"][::-1] and sorted(lists["every block doubled"]) == sorted(2 * list(range(n)))


def test_the_table_s_size():
    total = sum(len(s.data) for s in S.sources())
    assert total < 40 << 20 and max(len(s.data) for s in S.sources()) <= 130 * S.U
