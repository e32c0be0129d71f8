"""The planted parts of tests/buzhash_plants.py proved on the CPU, before tests/test_gpu_buzhash_plants.py sends them through the scans:
  - window_for gives any wanted hash (lto_buzhash_at), from the one copy of the table;
  - every part's candidate set under the oracle's own scan (lto_hpcdc_candidates) is exactly the planted one, and the oracle's chunks
    (lto_hpcdc_chunk_stream, and the position-pure form) are the lengths the plants spell out;
  - coverage is counted: the sweep's cuts fall in all 4096 (lane, step) classes of the tile scan's wave-tile and in all 4096 classes of
    the walking scan's tile, which starts at jump(qlo); every select arrangement is found again in the two-level bitmap;
  - walk_trace follows the walking scan over a part: the dense parts send it back to a tile behind a round, the guess parts leave a
    guess wrong, used for the jump behind a chunk of max bytes, or in flight at the part's end;
  - a numpy model of the scan's candidates and of the selection agrees with the oracle, and with one rule broken -- the halo dropped, the
    exact test skipped, the wrong test for the kind of d, qlo unmasked, a search that stops at a masked run or after 64 level-1 words --
    it answers differently on the cases that are there for that defect (no kernel is ever run broken);
  - the averages used for power-of-two discriminators give them under the oracle and under the reference's formula;
  - the reference library itself cuts the planted parts where the oracle does (live where oracle/_ref is built, recorded elsewhere)."""
import ctypes as C

import numpy as np
import pytest

from tests import buzhash_plants as P
from tests._libs import digest

M32 = P.M32


def test_the_table_is_the_oracle_s():
    from tests._libs import oracle

    t = (C.c_uint32 * 256).in_dll(oracle().dll, "lto_buzhash_table")
    assert list(t) == P.TABLE.tolist()
    z = np.zeros(48, np.uint8)
    assert P.buzhash(z) == P.ZERO_HASH == int(oracle().dll.lto_buzhash_at(z.ctypes.data, 48))


def test_window_for_hits_any_hash(oracle):
    rng = np.random.default_rng(5)
    targets = [0, M32, 1, 0x80000000, P.ZERO_HASH] + [d - 1 for d in P.DIV_EDGE_CFGS] + [int(x) for x in rng.integers(0, 1 << 32, 40)]
    for t in targets:
        w = P.window_for(t, rng)
        buf = np.concatenate([rng.integers(0, 256, 7, dtype=np.uint8), w])
        assert len(w) == 48 and w.dtype == np.uint8
        assert int(oracle.dll.lto_buzhash_at(buf.ctypes.data, len(buf))) == t == P.buzhash(w)
    a = rng.integers(0, 256, 5000, dtype=np.uint8)
    h = P.hashes(a)
    assert all(int(h[p - 48]) == int(oracle.dll.lto_buzhash_at(a.ctypes.data, p)) for p in (48, 49, 100, 4095, 4096, 4097, 5000))


def test_power_of_two_averages(oracle):
    for avg, d in P.POW2_AVERAGES.items():
        assert int(oracle.dll.lto_hpcdc_discriminator(avg)) == d == P.reference_discriminator(avg) and P.is_pow2(d), avg
    for cfgs in (P.SWEEP_CFGS, P.HEADLINE_CFGS, P.SELECT_FAR_CFGS, P.DENSE_CFGS):
        assert [P.is_pow2(P.disc(av)) for _, av, _ in cfgs] == [False, True]  # each case in both kinds of d
    assert [P.disc(c[1]) for c in P.DIV_EDGE_CFGS.values()] == list(P.DIV_EDGE_CFGS)
    assert [P.disc(c[1]) for c in P.SWEEP_CFGS + P.HEADLINE_CFGS] == [525, 512, 24680, 16384]


def test_a_part_that_cannot_be_exact_is_a_builder_error():
    with pytest.raises(AssertionError):
        P.planted_part(400, [(200, 7)], 64)  # 7 is no candidate for 64
    with pytest.raises(AssertionError):
        P.planted_part(400, [], 64, decoys=[(200, 63)])  # and 63 is one
    with pytest.raises(AssertionError):
        P.planted_part(400, [401], 64)


def lens_of(case_name, gi, pi):
    return P.expected(case_name)[gi][pi][1].tolist()


def test_place_cycles_through_the_phases():
    parts = [np.zeros(n, np.uint8) for n in (5, 0, 100, 64, 17, 1, 4096, 33)]
    offs, total = P.place(parts)
    assert [o % 64 for o in offs] == [0, 16, 32, 48] * 2 and total >= offs[-1] + 33
    assert all(offs[i] + len(parts[i]) <= offs[i + 1] for i in range(7))


@pytest.mark.parametrize("name", ["sweep", "sparse_sweep"])
def test_sweeps_are_exact_and_cover_every_class(oracle, name):
    case = P.CASES[name]()
    tile, walk, starts, aligns = set(), set(), set(), set()
    for gi, g in enumerate(case.groups):
        mn, av, mx = g.cfg
        d = P.disc(av)
        for pi, (part, (L, dist)) in enumerate(zip(g.parts, g.labels)):
            assert P.candidates(part, d).tolist() == [L, L + dist]
            assert lens_of(name, gi, pi) == [L, dist, len(part) - L - dist] and 0 < len(part) - L - dist <= mn
            if gi == 0:
                s = 0
                for p in (L, L + dist):  # the chunk from s ends at p: candidate bit q = p - 1, the walk's tile from jump(s + min)
                    q, tb = p - 1, P.jump(s + mn)
                    assert tb <= s + mn < tb + 16 and tb % 16 == 0
                    tile.add(q % P.WTILE)
                    walk.add((q - tb) % P.WTILE)
                    aligns.add(s + mn - tb)
                    s = p
                starts.add(L % 16)
        assert g.labels == case.groups[0].labels  # the same cuts for both kinds of d
    if name == "sweep":
        assert starts == set(range(16)) and aligns == set(range(16))  # the second chunk's start, and its tile against its first candidate
        assert len(tile) == 4096 and len(walk) == 4096, (len(tile), len(walk))
        first = {L - 1 for L, _ in case.groups[0].labels}
        assert first == set(range(512, 512 + 4160))  # every class by the first cut alone, and the crossing into the next tile
        assert {(q - P.jump(512)) % 4096 for q in first} == set(range(4096)) and P.jump(512) == 512
    else:
        classes = {(lane, step) for lane in P.SPARSE_LANES for step in P.SPARSE_STEPS}
        first = [L - 1 for L, _ in case.groups[0].labels]
        assert len(first) == 3 * len(classes) == 273
        assert {((q % 4096) // 64, q % 64) for q in first[:91]} == classes  # from min = a tile's start: lane and step as named
        assert {q >> 12 for q in first[91:182]} == {2, 3} and {q >> 14 for q in first[182:]} == {0, 1}  # across 12288, across 16384
        assert {((q - 2048) % 4096 // 64, q % 64) for q in first[91:]} == classes


def test_div_edges_plant_the_hashes_they_name(oracle):
    case = P.div_edges()
    assert [P.disc(g.cfg[1]) for g in case.groups] == [24680, 96, 75, 49535, 64, 16384]
    for gi, g in enumerate(case.groups):
        mn, av, mx = g.cfg
        d = P.disc(av)
        k2 = (d & -d).bit_length() - 1
        dodd = d >> k2
        cuts, decoys = P.div_edge_hashes(d)
        assert cuts["H+1 = d"] + 1 == d and (cuts["H+1 = the largest multiple of d"] + 1) % d == 0
        assert cuts["H+1 = the largest multiple of d"] + 1 + d > M32 >= cuts["H+1 = the largest multiple of d"]
        assert all(h % d == d - 1 for h in cuts.values()) and all(h % d != d - 1 for h in decoys.values())
        assert decoys["H = 0"] == 0 and decoys["H = d-2"] == d - 2
        if P.is_pow2(d):
            assert cuts["H = 0xFFFFFFFF"] == M32 and len(decoys) == 4
            for h in (decoys["low bits all ones but bit 0"], decoys["low bits all ones but the top one"]):
                assert bin(~h & (d - 1)).count("1") == 1
        else:
            assert decoys["H = 0xFFFFFFFF"] == M32  # passes the necessary test of every d: H + 1 = 0
            inv = pow(dodd, -1, 1 << 32)  # the necessary test: (H + 1) * inv mod 2^32 <= floor((2^32 - 1) / dodd)
            passes = [h for h in decoys.values() if ((h + 1) * inv) & M32 <= M32 // dodd]
            assert len(passes) == (3 if k2 else 1), (d, passes)  # necessary test passed, exact test failed
            if k2:
                assert {(h + 1) // dodd & 1 for h in passes if h != M32} == {1} and {24680: 3, 96: 5}[d] == k2
        assert len(g.parts) == len(cuts) + 1
        for pi, (part, (label, p, h, at)) in enumerate(zip(g.parts, g.labels)):
            assert [x for _, x in at] == list(decoys.values())
            assert P.candidates(part, d).tolist() == ([p] if p else [])
            for pos, want in at + ([(p, h)] if p else []):
                assert int(oracle.dll.lto_buzhash_at(part.ctypes.data, pos)) == want, (d, label, pos)
            assert all(mn < pos < (p or len(part)) for pos, _ in at)  # every decoy is a legal cut position in front of the cut
            assert lens_of("div_edges", gi, pi) == ([p, len(part) - p] if p else [len(part)])
            assert oracle.chunk(part, *g.cfg, pure=True).tolist() == lens_of("div_edges", gi, pi)


def bitmap(part, d):
    """The two levels as k_buzhash_prefix_dma leaves them: bit q of level 0 <=> a cut at q + 1; level 1 one bit per 64-byte run."""
    q = P.candidates(part, d) - 1
    return q, np.unique(q >> 6)


def test_select_arrangements_are_in_the_bitmap(oracle):
    case = P.select()
    seen = set()
    for gi, g in enumerate(case.groups):
        mn, av, mx = g.cfg
        d = P.disc(av)
        for pi, (part, (name, s)) in enumerate(zip(g.parts, g.labels)):
            q, runs = bitmap(part, d)
            lens = lens_of("select", gi, pi)
            assert oracle.chunk(part, *g.cfg, pure=True).tolist() == lens
            seen.add(name)
            if s:
                assert lens[0] == s and q[0] == s - 1
            qlo, qhi = s + mn, s + min(len(part) - s, mx) - 1
            legal = q[(q >= qlo) & (q <= qhi)]
            cut = s + lens[1 if s else 0] - 1  # the candidate bit that ends the chunk at issue
            if name.startswith("decoy at min"):
                assert qlo - 1 in q and (qlo - 1) >> 6 == qlo >> 6 and qlo % 64 == 20  # a flagged first run with a bit below qlo
                assert legal[0] == cut and lens[1] > mn
                if "same run" in name:
                    assert cut == qlo
                elif "later run" in name:
                    assert cut >> 6 > qlo >> 6 and cut >> 12 == qlo >> 12 and not ((q >> 6) == (qlo >> 6))[q >= qlo].any()
                elif "later word" in name:
                    assert cut >> 12 == (qlo >> 12) + 1
                else:
                    assert (cut >> 12) - (qlo >> 12) >= 64 and cut - qlo > 262144 and mx == 524288  # the second trip of the search
            elif name == "two candidates in one run":
                assert len(legal) == 2 and legal[0] >> 6 == legal[1] >> 6 and cut == legal[0] == qlo
            elif name.startswith("candidate at max+1"):
                bit = int(name.split()[-1])
                assert qhi % 64 == bit and qhi + 1 in q and len(legal) == 0 and lens[1] == mx
                assert ((qhi + 1) >> 6 == qhi >> 6) == (bit != 63)  # masked in the last run's word, or in level 1
            elif name.startswith("candidate at max"):
                assert cut == qhi == s + mx - 1 and qhi % 64 == int(name.split()[-1]) and lens[1] == mx and list(legal) == [qhi]
            elif name.startswith("candidate at size"):
                assert cut == qhi == len(part) - 1 and lens[1] < mx and len(lens) == 2
            else:
                assert name.startswith("cut on bit") and s == 0
                bit, run = int(name.split()[3]), int(name.split()[6])
                assert cut % 64 == bit and (cut >> 6) % 64 == run and list(legal) == [cut]
    assert len(seen) == 4 + 1 + 6 + 4


def test_dense_and_guess_are_what_they_claim(oracle):
    for gi, g in enumerate(P.dense().groups):
        d = P.disc(g.cfg[1])
        for pi, (part, gaps) in enumerate(zip(g.parts, g.labels)):
            assert len(gaps) == 150 > 64 and min(gaps) >= 65 and max(gaps) <= 200 and len(set(gaps)) > 50
            assert P.candidates(part, d).tolist() == np.cumsum(gaps).tolist()
            assert lens_of("dense", gi, pi) == gaps + [len(part) - sum(gaps)]
            per_tile = np.bincount(np.cumsum(gaps) >> 12)
            assert per_tile.max() >= 25  # many cuts in one 4 KiB tile
    for gi, g in enumerate(P.guess().groups):
        mn, av, mx = g.cfg
        d = P.disc(av)
        for pi, (part, (kind, L, k)) in enumerate(zip(g.parts, g.labels)):
            lens, cand = lens_of("guess", gi, pi), P.candidates(part, d).tolist()
            if kind == "tail":  # the cut, then a chunk that needs no scan
                assert lens == [L, k] and k <= mn and cand == [L]
            elif kind == "max":  # the cut, a chunk that ends at max, a cut again (the guess aimed at the next tile), the tail
                assert lens[:3] == [L, mx, mn + k] and cand == [L, L + mx + mn + k] and lens[3] <= mn
            else:
                assert lens == [mx, mn] and cand == []


def traces(name, hashing=True):
    return [[P.walk_trace(lens_of(name, gi, pi), len(p), g.cfg[0], g.cfg[2], hashing) for pi, p in enumerate(g.parts)]
            for gi, g in enumerate(P.CASES[name]().groups)]


def test_the_walk_takes_the_paths_the_cases_are_there_for():
    """walk_trace follows walk_body over the oracle's chunks of a part (it fails if the walk would emit another length)."""
    for group in traces("dense"):
        for t in group:  # several cuts per tile, and the pending list fills inside a tile: that tile again behind the round
            assert t["rehash"] >= 2 and t["same_tile"] >= 100 and t["tiles"] < 20
    for group in traces("dense", hashing=False):
        assert all(t["rehash"] == 0 and t["same_tile"] >= 140 for t in group)
    for g, group in zip(P.guess().groups, traces("guess")):
        by = {label: t for label, t in zip(g.labels, group)}
        mn, mx = g.cfg[0], g.cfg[2]
        # a cut under a guess aimed at the next 4 KiB, then a tail that needs no scan: the guess is in flight when the part is done
        for label in (("tail", mn + 1001, mn), ("tail", mn + 1, mn - 1)):
            assert by[label] == dict(tiles=1, same_tile=0, rehash=0, used_next=0, used_jump=0, wrong=0, wasted=1), label
        assert by[("tail", mn + 1001, 1)]["wasted"] == 0 and by[("tail", mn + 5000, 77)]["used_next"] == 1  # (no guess; a right one)
        for label, t in by.items():
            if label[0] == "max":  # the cut makes the guess wrong; the chunk of max bytes ends under a guess at the jump behind it, used
                assert t["wrong"] == 1 and t["used_jump"] == 1 and t["used_next"] >= 29 and t["wasted"] == 1, (label, t)
        assert by[("max then tail", mx, mn)]["used_jump"] == 0 and by[("max then tail", mx, mn)]["wasted"] == 0  # the guess is not aimed
    same = sum(t["same_tile"] for t in traces("sweep")[0])
    assert same > 3000  # min < 4 KiB: the second chunk's first candidate mostly lies in the tile that held the first cut
    assert sum(t["wrong"] for t in traces("sparse_sweep")[0]) > 200  # headline parameters: a cut, then a jump the guess did not foresee


def test_from_buffer_plants_cut_behind_the_quirk_zone(oracle):
    plants = P.from_buffer_plants()
    assert len(plants) == 9 and {p - cfg[0] for cfg, _, p in plants} == {48, 49, 111}
    for cfg, a, p in plants:
        assert P.is_pow2(P.disc(cfg[1])) and p < min(len(a), cfg[2]) and not a[: p - 48].any() and not a[p:].any()
        assert int(oracle.dll.lto_hpcdc_next_from_buffer(a.ctypes.data, len(a), *cfg)) == p
        assert P.is_candidate(P.buzhash(a[p - 48 : p]), P.disc(cfg[1]))


# ---- the model, sound and broken -------------------------------------------------------------------------------------------------------------


def model_parts():
    """(case, group index, part index): every part of the small cases, and of the sweeps the parts whose first cut sits in lane 0 below
    step 47 of a tile that is not the part's first (the halo), plus every 97th."""
    out = []
    for name in ("div_edges", "select", "dense", "guess"):
        out += [(name, gi, pi) for gi, g in enumerate(P.CASES[name]().groups) for pi in range(len(g.parts))]
    for name in ("sweep", "sparse_sweep"):
        for gi, g in enumerate(P.CASES[name]().groups):
            out += [(name, gi, pi) for pi, (L, _) in enumerate(g.labels) if ((L - 1) % 4096 < 47 and L > 4096) or pi % 97 == 0]
    return out


@pytest.fixture(scope="module")
def model_answers():
    """flags -> {part: whether the model's lengths are the oracle's}."""
    answers = {}
    sound = {}
    for key in model_parts():
        name, gi, pi = key
        g = P.CASES[name]().groups[gi]
        part, (mn, av, mx) = g.parts[pi], g.cfg
        d = P.disc(av)
        want = lens_of(name, gi, pi)
        sound[key] = P.model_candidates(part, d)
        answers.setdefault((), {})[key] = P.model_select(sound[key], len(part), mn, mx).tolist() == want
        for m in P.MUTANTS:
            cand = sound[key] if m in ("qlo_unmasked", "stop_at_masked_run", "one_trip") else P.model_candidates(part, d, (m,))
            answers.setdefault(m, {})[key] = P.model_select(cand, len(part), mn, mx, (m,)).tolist() == want
    return answers


def test_the_sound_model_agrees_with_the_oracle(model_answers):
    assert len(model_answers[()]) > 250 and all(model_answers[()].values())


def caught_in(model_answers, mutant):
    return {f"{name}:{P.CASES[name]().groups[gi].labels[pi][0]}" if name in ("select", "div_edges") else name
            for (name, gi, pi), same in model_answers[mutant].items() if not same}


def test_every_mutant_is_caught(model_answers):
    caught = {m: caught_in(model_answers, m) for m in P.MUTANTS}
    assert all(caught[m] for m in P.MUTANTS), {m: len(c) for m, c in caught.items()}
    assert {"sweep", "sparse_sweep", "select:cut on bit 0 of run 0"} <= caught["no_halo"]
    assert {"div_edges:H+1 = d", "div_edges:decoys alone"} <= caught["skip_exact"]
    assert {"sweep", "sparse_sweep", "dense", "guess"} <= caught["mask_for_any_d"]
    assert caught["general_for_pow2"] == {"div_edges:H = 0xFFFFFFFF"}  # the one hash the general test gets wrong for a power of two
    decoy = "select:decoy at min, cut "
    assert {decoy + "at min+1 in the same run", decoy + "in a later run of the same word", decoy + "in a later word",
            decoy + "more than 256 KiB behind"} <= caught["qlo_unmasked"]
    assert caught["stop_at_masked_run"] == {decoy + "in a later run of the same word", decoy + "in a later word", decoy + "more than 256 KiB behind"}
    assert caught["one_trip"] == {decoy + "more than 256 KiB behind"}


def test_mutants_are_caught_for_both_kinds_of_d(model_answers):
    for m in ("no_halo", "qlo_unmasked", "stop_at_masked_run", "one_trip"):
        kinds = {P.is_pow2(P.disc(P.CASES[name]().groups[gi].cfg[1])) for (name, gi, pi), same in model_answers[m].items() if not same}
        assert kinds == {False, True}, m


def test_the_reference_cuts_the_planted_parts_where_the_oracle_does(refcall):
    """The reference library is the specification; the oracle's lengths of every planted part are the reference's own (its streaming
    chunker through a feeder), so the GPU tests hold the kernels to the reference's answer."""
    for name in P.CASES:
        case = P.CASES[name]()
        mine = [[r[1].tolist() for r in res] for res in P.expected(name)]
        inputs = [digest(*g.parts) for g in case.groups] + [g.cfg for g in case.groups]
        want = refcall("plants.chunk_lens." + name, inputs,
                       lambda r: digest([[r.chunk_and_hash(p, *g.cfg)[1].tolist() for p in g.parts] for g in case.groups]))
        assert digest(mine) == want, name
