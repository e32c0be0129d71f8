"""The keys of tests/hash_table_keys.py proved on the CPU, before tests/test_gpu_hash_table_keys.py sends them through the device tables:
  - unmix64 inverts mix64, key_at gives the home slot it promises at every table size, and no builder emits 0 or all-ones unasked;
  - through the sequential TableModel every named case reaches the corner it claims: the probe that crosses the end of the table, the
    probe of 299 / 511 slots, the absent key's walk over a whole cluster, the reinsert across the end at every size a table grows to,
    all at a load of one half or less;
  - a model with one rule broken on purpose -- a find that stops at the first other key, a probe step without the wrap, a growth that
    drops a pair whose slot is taken, a value that is the last and not the smallest, a distinct count that looks at lane 0 alone -- gives
    another answer than the sound model on the cases that are there for that defect (no kernel is ever run broken);
  - the hash the model uses is the one in the two .hip sources;
  - where oracle/_ref is built: the reference treats the hashes 0 and all-ones as ordinary hashes in the two store-index calls."""
from pathlib import Path

import numpy as np
import pytest

from tests import hash_table_keys as K

ROOT = Path(__file__).resolve().parent.parent
SOURCES = ("longtail_amd/csrc/k_dedup.hip", "longtail_amd/csrc/version_index.hip")


def test_unmix64_inverts_mix64():
    rng = np.random.default_rng(1)
    words = [0, K.M64, 1, 1 << 63] + [int(x) for x in rng.integers(0, 2**64, 1000, dtype=np.uint64)]
    for x in words:
        assert K.unmix64(K.mix64(x)) == x and K.mix64(K.unmix64(x)) == x
    assert K.mix64(0) == 0  # hash 0 lives at home slot 0
    assert (K.MUL1 * K.INV1) & K.M64 == 1 and (K.MUL2 * K.INV2) & K.M64 == 1


def test_key_at_gives_the_promised_home_at_every_size():
    rng = np.random.default_rng(2)
    for home, j in [(0, 1), (1023, 0), ((1 << 20) - 1, 5), (8191, 100)] + [(int(h), int(j)) for h, j in rng.integers(0, 1 << 20, (200, 2))]:
        k = K.key_at(home, j)
        for bits in range(10, 21):
            assert K.mix64(k) & ((1 << bits) - 1) == home & ((1 << bits) - 1)
    a, b = K.key_at(5, 1), K.key_at(5 + 1024, 1)  # homes 1024 apart: together in 1024 slots, apart in 2048
    assert K.mix64(a) & 1023 == K.mix64(b) & 1023 and K.mix64(a) & 2047 != K.mix64(b) & 2047
    assert [K.slots_for(n) for n in (0, 1, 512, 513, 1024, 1025, 4096)] == [1024, 1024, 1024, 2048, 2048, 4096, 8192]


def plain_cases():
    out = []
    for S in (1024, 2048):
        out += [K.wrap(S), K.one_home(S), K.half_full_one_home(S), K.absent(S)]
    return out + [K.grow(True), K.grow(False), K.lone_claim()]


def test_no_builder_emits_zero_or_all_ones_unasked():
    for c in plain_cases():
        assert len(c.hashes) <= 4096 and 0 not in c.hashes and np.uint64(K.EMPTY) not in c.hashes, c.name
        assert all(q.key != 0 for q in c.queries)
    for S in (1024, 2048):
        s = K.specials(S)
        assert (s.hashes == 0).sum() == 3 and (s.hashes == np.uint64(K.EMPTY)).sum() == 4
        assert len(set(np.flatnonzero(s.hashes == 0) // 64)) > 1  # (in more than one wave)
    for c in (K.wrap(), K.one_home(), K.half_full_one_home(), K.specials()):
        for count in (600, 1024):
            h = K.padded(c, count)
            assert len(h) == count and K.slots_for(count) == 2048
            pad = np.setdiff1d(h, c.hashes)
            assert len(pad) == count - len(c.hashes) and 0 not in pad and np.uint64(K.EMPTY) not in pad


def run(case, **flags):
    return K.model_first_seen(case.calls or [case.hashes], case.slots, queries=[q.key for q in case.queries], **flags)


def final(case):
    r = run(case)
    return r, r["tables"][-1]


def test_every_case_stays_at_half_load_or_below():
    for c in plain_cases() + [K.specials(1024), K.specials(2048)]:
        r = run(c)
        pos = 0
        for call, t in zip(c.calls or [c.hashes], r["tables"]):
            pos += len(call)
            assert pos * 2 <= t.slots and t.load() <= 0.5, c.name  # (the count a table is sized from, and what it really holds)
        assert all(g.load() <= 0.5 for g in r["grows"])
    assert final(K.half_full_one_home())[1].load() == 0.5  # the densest table the sizing rule allows


@pytest.mark.parametrize("S", [1024, 2048])
def test_wrap_specials_and_half_full_cross_the_end(S):
    for c in (K.wrap(S), K.specials(S), K.half_full_one_home(S)):
        r, t = final(c)
        assert t.wrapped and t.slots == S, c.name
        first, n, wraps = K.cluster_of(c.hashes, S)
        assert wraps
        if c.name == "wrap":
            assert (first, n) == (S - 3, 50) and t.longest >= 40
        if c.name == "specials":  # one slot more: hash 0's; in the sequential model it finds its home taken by a key that wrapped
            assert (first, n) == (S - 3, 51) and t.find(0)[1].passed >= 1
        if c.name == "half_full_one_home":
            assert (first, n) == (S - 1, 512) and t.longest == 511


@pytest.mark.parametrize("S", [1024, 2048])
def test_one_home_probes_299_slots(S):
    c = K.one_home(S)
    r, t = final(c)
    assert t.longest == 299 and len(c.hashes) == 450 and len(np.unique(c.hashes)) == 300
    assert K.cluster_of(c.hashes, S) == (S // 2, 300, False)
    first, distinct = K.first_occurrence(c.hashes)
    assert r["answers"] == first.tolist() and r["distinct"] == [distinct]  # (the sound model agrees with numpy)


@pytest.mark.parametrize("S", [1024, 2048])
@pytest.mark.parametrize("table", ["absent", "half_full_one_home", "specials"])
def test_absent_queries_walk_to_the_empty_slot_behind_the_cluster(S, table):
    c = K.absent(S) if table == "absent" else getattr(K, table)(S)
    queries = c.queries or K.absent_queries(c.hashes, S)
    labels = [q.label for q in queries]
    assert len(queries) == (5 if table == "specials" else 6) and ("all-ones before it was ever added" in labels) == (table != "specials")
    t = final(c)[1]
    n = K.cluster_of(c.hashes, S)[1]
    for q in queries:
        assert q.key not in [int(h) for h in c.hashes]
        value, walk = t.find(q.key)
        assert value is None and walk.passed == q.min_passed and walk.wrapped == q.crosses, (q.label, walk)
    by = {q.label: q for q in queries}
    assert by["the cluster's first slot"].min_passed == n and by["the cluster's first slot"].crosses
    assert by["the cluster's middle"].min_passed == n - n // 2
    assert by["slot S-1, the cluster wrapped"].crosses and by["slot S-1, the cluster wrapped"].min_passed >= 47
    assert by["the empty slot just after the cluster"].min_passed == by["the slot just before the cluster"].min_passed == 0


@pytest.mark.parametrize("skip", [True, False])
def test_grow_reinserts_across_the_end_at_every_size(skip):
    c = K.grow(skip)
    r = run(c)
    sizes = [2048, 8192] if skip else [2048, 4096, 8192]
    assert [g.slots for g in r["grows"]] == sizes and len(c.hashes) == 4096
    assert [t.slots for t in r["tables"]] == c.notes["sizes"] and c.notes["sizes"][0] == 1024 and c.notes["sizes"][-1] == 8192
    for g in r["grows"]:  # the reinsertion alone: pairs that still collide in the new table, and a walk from its last slot to slot 0
        assert g.wrapped and g.longest > 16, g.slots  # (16: the longest probe the suite's random keys ever made)
    for t in r["tables"]:  # ... and the inserts of every call at every size
        assert t.wrapped and t.longest > 16, t.slots
    first, distinct = K.first_occurrence(c.hashes)
    assert r["answers"] == first.tolist() and r["distinct"][-1] == distinct
    # the absent queries rebuilt for each size find a wrapped cluster there
    pos = 0
    for call, t in zip(c.calls, r["tables"]):
        pos += len(call)
        q = K.absent_queries(c.hashes[:pos], t.slots)
        assert len(q) == 6 and all(t.find(x.key) == (None, K.Walk(x.min_passed, x.crosses)) for x in q)
        q8 = K.absent_queries(c.hashes[:pos], 8192)  # (for the table made for all of them, which never grows)
        assert len(q8) == 6 and q8[0].crosses
    # pairs with homes 1024 apart are in: together at 1024 slots, apart at 2048
    homes = np.array([K.mix64(int(h)) & ((1 << 20) - 1) for h in np.unique(c.hashes)])
    assert len(np.intersect1d(homes[homes < 1024] + 1024, homes)) >= 30


def test_lone_claim_is_one_claiming_lane_per_call():
    c = K.lone_claim()
    assert len(c.notes["subs"]) == 21 and {n for n, p in c.notes["subs"]} == set(K.LONE_N)
    assert {(63, 62), (64, 63), (65, 64), (256, 255), (257, 256), (257, 255), (1, 0)} <= set(c.notes["subs"])
    r = run(c)
    assert r["distinct"] == list(range(1, len(c.calls) + 1))
    for (n, p), call in zip(c.notes["subs"], c.calls[1:]):
        assert len(call) == n and (call != call[(p + 1) % n]).sum() == (1 if n > 1 else 0) and (n == 1 or call[p] != call[(p + 1) % n])


# ---- each case would notice the defect it is there for --------------------------------------------------------------------------------


def answers_differ(case, **flags):
    good, bad = run(case), run(case, **flags)
    if bad == K.LEFT:
        return True
    return any(good[k] != bad[k] for k in ("answers", "distinct", "queries"))


def test_a_find_that_stops_at_the_first_other_key_is_noticed():
    for c in (K.wrap(), K.one_home(), K.half_full_one_home(), K.specials(), K.grow(True)):
        assert answers_differ(c, find_stops=True), c.name


def test_a_probe_step_without_the_wrap_is_noticed():
    for c in (K.wrap(), K.specials(), K.half_full_one_home(), K.absent(), K.grow(True), K.grow(False)):
        assert run(c, no_wrap=True) == K.LEFT, c.name
    assert run(K.one_home(), no_wrap=True) != K.LEFT  # (the case that stays in the middle of the table does not reach this)
    # the absent query of home S-1 alone, against a sound table
    t = K.TableModel(1024, no_wrap=True)
    t.keys, t.vals = final(K.absent())[1].keys, final(K.absent())[1].vals
    with pytest.raises(K.Left):
        t.find(K.absent().queries[4].key)


def test_a_growth_that_drops_a_pair_whose_slot_is_taken_is_noticed():
    for skip in (True, False):
        c = K.grow(skip)
        good, bad = run(c), run(c, reinsert_drops=True)
        assert good["answers"] != bad["answers"] and good["distinct"] != bad["distinct"]  # a lost key is claimed again by its repeat


def test_a_value_that_is_the_last_and_not_the_smallest_is_noticed():
    for c in (K.wrap(), K.one_home(), K.specials(), K.grow(True), K.lone_claim()):
        assert answers_differ(c, keep_last=True), c.name
    for c in (K.wrap(), K.one_home(), K.specials()):  # ... and with the ordinals of the min_ordinal tests, whatever the order of arrival
        o = K.ordinals_for(c.hashes)
        for order in (slice(None), slice(None, None, -1)):
            h, v = c.hashes[order], o[order]
            want = K.min_per_hash(h, v)[0].tolist()
            assert K.model_first_seen([h], c.slots, values=v)["answers"] == want
            assert K.model_first_seen([h], c.slots, values=v, keep_last=True)["answers"] != want


def test_a_distinct_count_that_looks_at_lane_0_alone_is_noticed():
    c = K.lone_claim()
    good, bad = np.diff(run(c)["distinct"]), np.diff(run(c, lane0_only=True)["distinct"])
    assert (good == 1).all()
    for (n, p), b in zip(c.notes["subs"], bad):
        assert b == (1 if p % 64 == 0 else 0), (n, p)
    assert sum(p % 64 != 0 for n, p in c.notes["subs"]) == 11  # (lanes 62, 63 and 255 of every n that has them)
    for c in (K.wrap(), K.one_home(), K.specials(), K.grow(True)):
        assert run(c)["distinct"] != run(c, lane0_only=True)["distinct"], c.name


def test_ordinals_put_the_minimum_in_the_middle():
    for c in (K.wrap(), K.one_home(), K.specials(), K.half_full_one_home()):
        o = K.ordinals_for(c.hashes).astype(np.int64)
        assert len(np.unique(o)) == len(o) and o.max() <= 2**31 - 2 and (o > 2**30).sum() > len(o) // 4
        middle = ends = 0
        for h in np.unique(c.hashes):
            at = np.flatnonzero(c.hashes == h)
            low = at[np.argmin(o[at])]
            if len(at) >= 3:
                assert low not in (at[0], at[-1])
                middle += 1
            elif len(at) == 2:
                ends += 1
        assert c.name == "half_full_one_home" or (middle >= 4 and ends >= 4)
        assert (o != np.arange(len(o))).any()


# ---- the model is in step with the sources ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("source", SOURCES)
def test_the_model_hashes_like_the_source(source):
    """If this fails, the table's hash or its smallest size changed in `source`: update MUL1 / MUL2 / INV1 / INV2 / SHIFT / MIN_SLOTS in
    tests/hash_table_keys.py, or the keys of the GPU cases no longer land where they aim."""
    text = (ROOT / source).read_text()
    compact = text.replace(" ", "")
    assert f"0x{K.MUL1:016x}ull" in text and f"0x{K.MUL2:016x}ull" in text, source
    assert compact.count(f"(z^(z>>{K.SHIFT}))*") == 2 and f"returnz^(z>>{K.SHIFT});" in compact, source
    assert f"uint64_t slots = {K.MIN_SLOTS};" in text and "slots <<= 1;" in text, source
    assert "0xFFFFFFFFFFFFFFFFull" in text and "(slot + 1) & mask" in text, source


# ---- the reference and the two special hashes ---------------------------------------------------------------------------------------------


def dict_existing(blocks, wanted, percent):
    """Longtail_GetExistingStoreIndex in sets: the blocks that hold wanted chunks, most used first, each taken when it brings a wanted
    chunk that no block before it brought."""
    w, ranked = {int(h) for h in wanted}, []
    for i, (_, _, chunks, sizes) in enumerate(blocks):
        use = sum(int(s) for h, s in zip(chunks, sizes) if int(h) in w)
        if use and not (percent and use * 100 // int(sizes.sum()) < percent):
            ranked.append((-(use * 100 // int(sizes.sum())), i))
    have, taken = set(), []
    for _, i in sorted(ranked):
        new = ({int(h) for h in blocks[i][2]} & w) - have
        if new:
            taken.append(blocks[i][0])
            have |= new
    return taken


def test_the_store_index_blocks_are_what_their_names_say():
    blocks, wanted = K.store_index_inputs()
    assert len(wanted["all"]) <= 512 and {0, K.EMPTY} <= {int(h) for h in wanted["all"]}
    a, b, c, d = (blocks[i][0] for i in range(4))
    for percent, want in ((0, True), (1, True), (50, True), (100, False)):
        taken = dict_existing(blocks, wanted["all"], percent)
        assert (a in taken) == want and b not in taken and (c in taken) == want and d in taken and taken[0] == d
    assert b in [x for x, _ in [(blk[0], 0) for blk in blocks]] and K.EMPTY in [int(h) for h in blocks[1][2]]
    assert b not in dict_existing(blocks, wanted["all-ones not wanted"], 0) and c in dict_existing(blocks, wanted["all-ones not wanted"], 0)
    assert dict_existing(blocks, wanted["all-ones alone"], 0) == [b] and dict_existing(blocks, wanted["all-ones alone"], 50) == []
    # absent chunks of the blocks have their homes inside the wanted set's clusters and at S-1
    t = K.TableModel(1024)
    for h in wanted["all"]:
        t.insert(int(h), 0)
    walks = [t.find(int(h)) for blk in blocks for h in blk[2] if int(h) not in {int(x) for x in wanted["all"]}]
    assert all(v is None for v, _ in walks) and max(w.passed for _, w in walks) >= 100 and any(w.wrapped for _, w in walks)


def test_the_reference_treats_0_and_all_ones_as_ordinary_hashes(ref):
    """The reference library is the specification of the two store-index calls; on the inputs of the GPU tests it agrees with the
    set arithmetic above and below, the hashes 0 and 0xFFFF...FFFF included, so its bytes are an expectation with nothing special in
    them."""
    blocks, wanted = K.store_index_inputs()
    blob = K.store_index_blob(blocks)
    for name, w in wanted.items():
        for percent in (0, 1, 50, 100):
            got = K.store_index_hashes(ref.get_existing_store_index(blob, w, percent))[0]
            assert got.tolist() == dict_existing(blocks, w, percent), (name, percent)
    for kind in K.MISSING_KINDS:
        for where in K.MISSING_WHERE:
            repeated = K.missing_content_inputs(kind, where)
            for inp in (K.missing_content_inputs(kind, where, repeats=False), K.first_occurrences(repeated)):
                want = version_minus_store(inp)
                assert K.store_index_hashes(K.ref_missing_content(ref, inp))[1].tolist() == want, (kind, where)
                assert {0, K.EMPTY} & set(want) == ({0, K.EMPTY} if where == "version" else set())


def version_minus_store(inp):
    have, want = {int(h) for h in inp["existing"]}, []
    for h in inp["hashes"]:
        if int(h) not in have:
            want.append(int(h))
            have.add(int(h))
    return want


def reference_on_repeats(inp):
    """What Longtail_CreateMissingContent makes of a version list with repeats, in sets and lists: the chunk hashes of its answer."""
    store, v = {int(h) for h in inp["existing"]}, [int(h) for h in inp["hashes"]]
    added = sorted(set(v) - store)
    walk = [h for h in v[: len(set(v))] if h not in store][: len(added)]  # as many ENTRIES as the list has distinct hashes
    walk += added[len(walk) :]  # where the walk wrote fewer than there are added hashes, the sorted ones stay behind it
    return list(dict.fromkeys(walk))  # Longtail_CreateStoreIndex keeps the first of equal hashes


def test_what_the_reference_makes_of_a_list_with_repeats(ref):
    """A VersionIndex's chunk list is unique by construction, and DiffHashes (src/longtail.c:6620-6743) relies on it: it counts the
    list's distinct hashes, then walks only that many ENTRIES of the list to put the added hashes back into version order (:6731).
    With r repeats the last r entries are never looked at, and a chunk that first occurs among them is left out of the missing content
    although the store lacks it: on each of the cluster inputs 18 to 22 of about 300 such chunks.  lthip_create_missing_content
    returns the same bytes (tests/test_gpu_hash_table_keys.py); this test holds the rule it mirrors against the reference itself."""
    lost = []
    for kind in K.MISSING_KINDS:
        for where in K.MISSING_WHERE:
            inp = K.missing_content_inputs(kind, where)
            want = version_minus_store(inp)
            got = K.store_index_hashes(K.ref_missing_content(ref, inp))[1].tolist()
            assert got == reference_on_repeats(inp) and set(got) < set(want), (kind, where)
            assert set(want) - set(got) <= {int(h) for h in inp["hashes"][len(np.unique(inp["hashes"])) :]}
            lost.append(len(want) - len(got))
    assert min(lost) == 18 and max(lost) == 22, lost
    short = full = 0
    for inp in K.mostly_repeats_inputs():
        got = K.store_index_hashes(K.ref_missing_content(ref, inp))[1].tolist()
        assert got == reference_on_repeats(inp)
        store, v = {int(h) for h in inp["existing"]}, [int(h) for h in inp["hashes"]]
        written = sum(h not in store for h in v[: len(set(v))])
        short += written < len(set(v) - store)  # sorted hashes stay behind the walk
        full += written > len(set(v) - store)  # the walk fills the list before its end
    assert short >= 5 and full >= 5
    for inp in (K.missing_content_inputs("wrap", "both", repeats=False), K.first_occurrences(K.mostly_repeats_inputs()[0])):
        assert reference_on_repeats(inp) == version_minus_store(inp)  # (a unique list: the rule is plain "version minus store")


@pytest.mark.parametrize("kind", K.MISSING_KINDS)
@pytest.mark.parametrize("where", K.MISSING_WHERE)
@pytest.mark.parametrize("repeats", [True, False])
def test_the_missing_content_inputs_fill_1024_slots_to_the_half(kind, where, repeats):
    inp = K.missing_content_inputs(kind, where, repeats)
    both = np.concatenate([inp["existing"], inp["hashes"]])
    assert len(both) == 512 and K.slots_for(len(both)) == 1024
    r = K.model_first_seen([both])
    t = r["tables"][0]
    assert t.longest >= {"wrap": 40, "one_home": 299, "half_full_one_home": 459}[kind] and (t.wrapped or kind == "one_home")
    e, v = inp["existing"], inp["hashes"]
    repeated = [h for h in np.unique(v) if (v == h).sum() > 1]
    if repeats:  # of a key the store holds, and of one it lacks
        assert any(h in e for h in repeated) and any(h not in e for h in repeated)
    else:
        assert repeated == [] and np.isin(v, e).sum() >= 20
    for s in (0, K.EMPTY):
        assert (np.uint64(s) in e) == (where != "version") and (np.uint64(s) in v) == (where != "store")
