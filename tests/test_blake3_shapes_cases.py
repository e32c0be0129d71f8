"""The case tables of tests/blake3_shapes.py, checked on the CPU: they hold every shape, residue and count that
tests/test_gpu_blake3_shapes.py iterates over, every range lies inside the source, and -- where the reference is built -- the oracle's
digests of the whole table are the reference's Blake3Hash_HashBuffer, so the expected values are not only our restatement."""
import numpy as np
import pytest

from tests import blake3_shapes as S
from tests._libs import ROOT as S_ROOT, have_ref, ref as get_ref

TABLES = {"small": S.small_table, "level": S.level_table, "one": S.one_table, "one_pinned": lambda: S.one_table(S.ONE_PINNED_RESIDUES)}


def test_constants():
    import re

    import longtail_amd.lib as lib

    h = (S_ROOT / "include" / "longtail_hip.h").read_text()
    assert int(re.search(r"#define LTHIP_B3_STREAM_BATCH \(1u << (\d+)\)", h).group(1)) == 20 and lib.B3_STREAM_BATCH == 1 << 20 == S.STREAM_BATCH
    assert int(re.search(r"#define LTHIP_B3_STREAM_STACK_BYTES (\d+)u", h).group(1)) == lib.B3_STREAM_STACK_BYTES
    for name in ("hash_one", "hash_runs_u64", "hash_runs_u64_bounded", "b3_stream"):
        assert callable(getattr(lib.Context, name))
    assert len(S.TAILS) == 14 and {t % 4 for t in S.TAILS} == {0, 1, 2, 3}
    assert {t % 64 for t in S.TAILS} >= {1, 63, 0} and {(t + 63) // 64 for t in S.TAILS} >= {1, 2, 16}
    assert len(S.N_SMALL) == 77 and set(range(1, 67)) <= set(S.N_SMALL) and max(S.N_SMALL) == 256 == S.WINDOW_MAX_LEN // S.KIB
    assert len(S.N_BIG) == 13 and min(S.N_BIG) == 257 and max(S.N_BIG) == 4097
    assert S.length(257, 1) == S.WINDOW_MAX_LEN + 1 and S.length(64, 1024) == 65536 and S.length(1, 0) == 0
    assert S.SRC_BYTES >= S.length(4097, 1024) + 16


@pytest.mark.parametrize("name,count,modulus,residues", [("small", 4316, 4, S.RANGE_RESIDUES), ("level", 578, 4, S.RANGE_RESIDUES),
                                                         ("one", 4485, 16, S.ONE_RESIDUES), ("one_pinned", 1794, 16, S.ONE_PINNED_RESIDUES)])
def test_tables_hold_every_shape_and_residue(name, count, modulus, residues):
    cases, offs, lens = TABLES[name]()
    assert len(cases) == len(offs) == len(lens) == count and len(set(cases)) == count
    assert all(int(l) == S.length(n, t) and int(o) % modulus == r for (n, t, r), o, l in zip(cases, offs, lens))
    assert (offs + lens <= S.SRC_BYTES).all()  # (and the source is SRC_PAD bytes longer: the last byte's aligned dword is inside)
    have = set(cases)
    ns = {"small": S.N_SMALL, "level": S.N_LEVEL, "one": S.N_ONE, "one_pinned": S.N_ONE}[name]
    full = [n for n in ns if n <= 256]  # the residue cross is full up to the window limit (level_table thins N_BIG only)
    assert have >= {(n, t, r) for n in full for t in S.TAILS for r in residues} | {(1, 0, r) for r in residues}
    assert {(n, t) for n, t, _ in cases} == {(n, t) for n in ns for t in S.TAILS} | {(1, 0)}
    for n in ns:
        assert {r for m, _, r in cases if m == n} == set(residues), n
    if name == "small":
        assert {(n, t) for n, t, _ in cases} >= {(n, t) for n in range(1, 67) for t in S.TAILS}
        assert int(np.sum([S.leaves(int(l)) for l in lens])) == 222324 == 4 * (1 + 14 * sum(S.N_SMALL))  # 218 windows of 1024 slots
    if name.startswith("one"):
        assert int(lens.max()) == 65536 and int(lens.min()) == 0
    # the starts are spread: ranges of one shape do not all begin at the source's first bytes
    assert len({int(o) // 16 for o in offs}) > count // 8


def test_stream_and_run_tables():
    sc = S.stream_cases()
    assert len(sc) == 92 == 1 + len(S.STREAM_B) * len(S.STREAM_TAILS) + 3 and len(set(sc)) == 92
    assert all(0 < t <= S.STREAM_BATCH for B, t in sc if B) and (0, 0) in sc and max(B * S.STREAM_BATCH + t for B, t in sc) <= S.STREAM_BYTES
    assert {bin(B).count("1") for B in S.STREAM_B} == {0, 1, 2, 3, 4}  # the stack's depth below the tail
    assert {((b + 1) & -(b + 1)).bit_length() - 1 for b in range(max(S.STREAM_B))} == {0, 1, 2, 3, 4}  # merges after batch b
    assert {S.leaves(t) for t in S.STREAM_TAILS} == {1, 2, 4, 5, 7, 8}
    sets = dict(S.run_sets())
    assert sorted(sets) == ["half", "t1024", "t128", "t64", "values"]
    half = np.diff(sets["half"])
    assert len(half) == 7 + 71 and int(half.max()) == 16264 and 2 * int(half.max()) * 8 <= S.WINDOW_MAX_LEN
    assert len(sets["values"]) == 37 and set(np.diff(sets["values"]).tolist()) == set(S.RUN_VALUES)
    for t in (64, 128, 1024):
        d = np.diff(sets[f"t{t}"])
        assert len(d) == 78 and d[0] == 0 and d[1:].tolist() == [S.length(n, t) // 8 for n in S.N_SMALL] and int(d.max()) * 8 <= S.WINDOW_MAX_LEN
    assert all(int(f[-1]) * 8 <= S.SRC_BYTES for f in sets.values())
    assert set(S.FUSED_M) == {1024, 1025, 3072, 3073, 65537} and S.FUSED_LEVEL == (300000, (1 << 20) + 5)
    assert S.STRADDLE_S == (767, 768, 769, 1022, 1023, 1024, 1025)


def test_window_scenarios_are_what_they_claim():
    sc = S.window_scenarios()
    assert len(sc) == 16 and [k for k in sc if k.startswith("straddle_")] == [f"straddle_{s}" for s in S.STRADDLE_S]
    total = lambda shapes: sum(n for n, _ in shapes)
    for s in S.STRADDLE_S:
        shapes = sc[f"straddle_{s}"]
        assert len(shapes) == s + 301 and shapes[s][0] == 256 and all(n == 1 for i, (n, _) in enumerate(shapes) if i != s)
        assert total(shapes[:s]) == s  # the large range's first slot: 1023 = the last of window 0, 1024 = the first of window 1
    # ranges * 8 < slots chooses how the window kernel fills its table
    branch = {k: len(sc[k]) * 8 < total(sc[k]) for k in ("4x256", "1024x1_every_fourth_empty", "128x8", "113x9", "146x7")}
    assert branch == {"4x256": True, "1024x1_every_fourth_empty": False, "128x8": False, "113x9": True, "146x7": False}
    assert all(total(sc[k]) <= S.PW for k in branch) and total(sc["128x8"]) == 1024 == len(sc["128x8"]) * 8
    assert sum(1 for n, t in sc["1024x1_every_fourth_empty"] if t == 0) == 256
    assert total(sc["total_2048"]) == 2048 and total(sc["total_2049"]) == 2049 and len(sc["one_range"]) == len(sc["one_empty_range"]) == 1
    for shapes in sc.values():
        cases, offs, lens = S.batch(shapes)
        assert [(n, t) for n, t, _ in cases] == shapes and all(int(o) % 4 == i % 4 for i, o in enumerate(offs))
        assert (offs + lens <= S.SRC_BYTES).all() and int(lens.max()) <= S.WINDOW_MAX_LEN


def test_first_mismatch_names_the_case():
    cases, _, _ = S.small_table()
    exp = np.arange(len(cases), dtype=np.uint64)
    assert S.first_mismatch(exp, exp, cases) == ""
    got = exp.copy()
    got[5] = 99
    n, t, r = cases[5]
    assert f"(n={n}, t={t}, residue={r}, position 5 in the batch)" in S.first_mismatch(got, exp, cases)
    order = np.arange(len(cases))[::-1]
    n, t, r = cases[int(order[5])]
    assert f"(n={n}, t={t}, residue={r}, position 5 in the batch)" in S.first_mismatch(got, exp, cases, order)


@pytest.mark.skipif(not have_ref(), reason="oracle/_ref/liblongtail_ref.so not built (needs /root/reference at build time)")
def test_oracle_equals_the_reference_on_the_whole_table(oracle):
    r = get_ref()
    src = S.source(oracle)
    for name in ("small", "level", "one"):
        cases, offs, lens = TABLES[name]()
        exp = oracle.blake3_many(src, offs, lens)
        for i, (o, l) in enumerate(zip(offs.tolist(), lens.tolist())):
            assert r.blake3(src[o : o + l]) == int(exp[i]), (name, S.what(cases, i))
    for _, first in S.run_sets():
        for a, b in zip(first[:-1].tolist(), first[1:].tolist()):
            assert r.blake3(src[8 * a : 8 * b]) == oracle.blake3(src[8 * a : 8 * b]), (a, b)
    stream = oracle.synth(S.STREAM_BYTES, S.SRC_SEED + 1, S.SRC_KIND)
    for B, t in S.stream_cases():
        n = B * S.STREAM_BATCH + t
        assert r.blake3(stream[:n]) == oracle.blake3(stream[:n]), (B, t)
