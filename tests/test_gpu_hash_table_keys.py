"""-m gpu: the device hash tables on keys built to collide, wrap and grow (tests/hash_table_keys.py; what each case reaches is proved on
the CPU in tests/test_hash_table_keys_cases.py).  The one-shot first-seen table (lthip_dedup_first_seen[_range], lthip_dedup_min_ordinal,
lthip_create_missing_content), lthip_seen, lthip_store and the second table of lthip_get_existing_store_index all get: a cluster that runs
over the end of the table, 300 and 512 keys of one home slot, the hashes 0 and 0xFFFF...FFFF inside a wrapped cluster, finds of absent
keys that must walk a whole cluster to the empty slot behind it, growth with keys that still collide in the larger table, and calls in
which one lane alone claims a slot.  Expected values are numpy's (first occurrence, isin, minimum per group) and, for the two
store-index calls, the reference library's bytes -- never the table model's."""
import functools

import numpy as np
import pytest
import torch

from longtail_amd.lib import Seen, Store
from tests import hash_table_keys as K

pytestmark = pytest.mark.gpu

EMPTY = K.EMPTY


def dev(h):
    return torch.from_numpy(np.ascontiguousarray(h, dtype=np.uint64).view(np.int64)).cuda()


def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().astype(np.int64)


@functools.lru_cache(maxsize=None)
def arrays():
    """name -> (hashes, the slots of a table sized for them).  Every case at 512 hashes or fewer (1024 slots), the four cluster cases
    again with their homes rebuilt for 2048 slots and padded with keys that collide nowhere to 513 .. 1024 hashes."""
    out = {}
    for c in (K.wrap(), K.one_home(), K.half_full_one_home(), K.specials()):
        out[c.name] = (c.hashes, 1024)
    for c, count in ((K.wrap(2048), 600), (K.one_home(2048), 1024), (K.half_full_one_home(2048), 1024), (K.specials(2048), 513)):
        out[c.name + "-2048"] = (K.padded(c, count), 2048)
    out["grow"] = (K.grow(True).hashes, 8192)
    out["lone_claim"] = (K.lone_claim().hashes, 8192)
    return out


ARRAYS = ("wrap", "one_home", "half_full_one_home", "specials", "wrap-2048", "one_home-2048", "half_full_one_home-2048", "specials-2048",
          "grow", "lone_claim")
CLUSTERS = {"wrap": K.wrap, "one_home": K.one_home, "half_full_one_home": K.half_full_one_home, "specials": K.specials}


def table_sizes(expected, sizes):
    """(slots, growths so far) after each of the calls, by the sizing rule of include/longtail_hip.h"""
    slots, grown, total, out = K.slots_for(expected), 0, 0, []
    for k in sizes:
        total += k
        if total * 2 > slots:
            slots, grown = K.slots_for(total), grown + 1
        out.append((slots, grown))
    return out


def queries_for(hashes, slots):
    """(query keys, numpy's isin): the absent queries aimed at the table's cluster, 40 more absent keys of homes inside it, and every
    third key the table holds"""
    first, n, _ = K.cluster_of(hashes, slots)
    absent = [q.key for q in K.absent_queries(hashes, slots)]
    inside = np.concatenate([K.absent_keys((first + d) & (slots - 1), 10) for d in (0, 1, n // 2, n - 1)])
    q = np.concatenate([np.array(absent, np.uint64), inside, np.unique(hashes)[::3]])
    q = q[np.random.default_rng(8).permutation(len(q))]
    want = np.isin(q, hashes)
    assert (~want).sum() >= len(absent) - 1 + 40 and want.sum() >= 1
    return q, want


# ---- the one-shot table -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ARRAYS)
def test_one_shot_first_seen(gpu, name):
    h, slots = arrays()[name]
    assert K.slots_for(len(h)) == slots
    want, distinct = K.first_occurrence(h)
    d = dev(h)
    first, uniq = gpu.dedup_first_seen(d)
    assert (host(first) == want).all() and int(uniq.item()) == distinct
    # a window of the look-ups that starts and ends inside a cluster (every hash of these arrays is a cluster's), and an empty one
    lo, count = len(h) // 3, len(h) // 3 + 1
    first, uniq = gpu.dedup_first_seen_range(d, lo, count)
    assert (host(first) == want[lo : lo + count]).all() and int(uniq.item()) == distinct
    first, uniq = gpu.dedup_first_seen_range(d, lo, 0)
    assert first.numel() == 0 and int(uniq.item()) == distinct


@pytest.mark.parametrize("name", ARRAYS)
def test_one_shot_min_ordinal(gpu, name):
    h, _ = arrays()[name]
    o = K.ordinals_for(h)
    assert int(o.max()) > 2**30 and int(o.max()) <= 2**31 - 2
    want, distinct = K.min_per_hash(h, o)
    first, uniq = gpu.dedup_min_ordinal(dev(h), dev32(o))
    assert (host(first) == want).all() and uniq == distinct


# ---- lthip_seen -------------------------------------------------------------------------------------------------------------------------


def seen_calls(gpu, calls, expected, check_finds):
    """The arrays of `calls` through one lthip_seen made for `expected` hashes: the concatenated first indexes and the running distinct
    count are numpy's, the growth count the sizing rule's; check_finds: after every call, finds of everything added so far and of the
    absent queries rebuilt for the table's size of the moment."""
    allh = np.concatenate(calls)
    want, _ = K.first_occurrence(allh)
    sizes = table_sizes(expected, [len(c) for c in calls])
    seen = Seen(gpu, expected)
    got, pos = [], 0
    for c, (slots, grown) in zip(calls, sizes):
        assert seen.total == pos
        first, d = seen.add(dev(c))
        pos += len(c)
        got.append(first)
        assert seen.grown == grown
        assert int(d.item()) == len(np.unique(allh[:pos]))
        if check_finds:
            sofar = allh[:pos]
            assert (host(seen.find(dev(sofar))) == K.first_occurrence(sofar)[0]).all(), (pos, slots)
            q = K.absent_queries(sofar, slots)
            assert (host(seen.find(dev([x.key for x in q]))) == -1).all(), (pos, slots, [x.label for x in q])
    gpu.sync()
    assert seen.total == len(allh) and (host(torch.cat(got)) == want).all()
    if check_finds:
        q, held = queries_for(allh, sizes[-1][0])
        position = host(seen.find(dev(q)))
        where = {int(k): i for i, k in reversed(list(enumerate(allh)))}
        assert (position == np.array([where.get(int(k), -1) for k in q])).all() and ((position >= 0) == held).all()
    seen.close()
    return sizes


@pytest.mark.parametrize("made_for_all", [False, True])
@pytest.mark.parametrize("name", ["wrap", "one_home", "half_full_one_home", "specials"])
def test_seen_calls_cut_inside_clusters(gpu, name, made_for_all):
    h = CLUSTERS[name]().hashes
    cuts = np.cumsum(K.cuts_inside(len(h)))[:-1]
    sizes = seen_calls(gpu, np.split(h, cuts), len(h) if made_for_all else 0, check_finds=True)
    assert sizes[-1] == (1024, 0)  # the size the homes are built for


@pytest.mark.parametrize("made_for_all", [False, True])
def test_seen_lone_claim(gpu, made_for_all):
    c = K.lone_claim()
    sizes = seen_calls(gpu, c.calls, len(c.hashes) if made_for_all else 0, check_finds=False)
    assert sizes[-1][0] == 8192 and sizes[-1][1] == (0 if made_for_all else 3)


@pytest.mark.parametrize("made_for_all", [False, True])
@pytest.mark.parametrize("skip", [True, False])
def test_seen_grows_with_keys_that_still_collide(gpu, skip, made_for_all):
    c = K.grow(skip)
    sizes = seen_calls(gpu, c.calls, len(c.hashes) if made_for_all else 0, check_finds=True)
    if made_for_all:
        assert sizes == [(8192, 0)] * len(c.calls)
    else:
        assert [s for s, _ in sizes] == c.notes["sizes"] and sizes[-1] == (8192, 2 if skip else 3)


# ---- lthip_store ------------------------------------------------------------------------------------------------------------------------


def chunk_index_of(h):
    """A StoreIndex blob whose chunk hashes are h, 64 to a block"""
    return K.store_index_blob([(0x2000 + i, 1, h[i : i + 64], np.full(len(h[i : i + 64]), 100, np.uint32)) for i in range(0, len(h), 64)])


def check_finds(store, hashes, slots):
    q, want = queries_for(hashes, slots)
    known, count = store.find(dev(q))
    assert (known.cpu().numpy() == want).all() and int(count.item()) == int(want.sum())
    # one hit among absent keys of the cluster's own homes, in the last lane of the call's last wave
    first, n, _ = K.cluster_of(hashes, slots)
    for k in (1, 63, 64, 65, 257):
        q = K.absent_keys((first + n // 2) & (slots - 1), k, K.FAR + 1000)
        q[k - 1] = hashes[len(hashes) // 2]
        known, count = store.find(dev(q), count=count)
        assert known.cpu().tolist() == [0] * (k - 1) + [1] and int(count.item()) == 1, k


@pytest.mark.parametrize("how", ["add", "add_index"])
@pytest.mark.parametrize("name", ["wrap", "one_home", "half_full_one_home", "specials"])
def test_store_membership_in_clusters(gpu, name, how):
    h = CLUSTERS[name]().hashes
    store = Store(gpu, 0)
    if how == "add":
        for c in np.split(h, np.cumsum(K.cuts_inside(len(h)))[:-1]):
            store.add(dev(c))
    else:
        store.add_index(chunk_index_of(h))
    assert store.added == len(h) and store.grown == 0 and store.distinct == len(np.unique(h))
    check_finds(store, h, 1024)
    if name == "specials":
        known, _ = store.find(dev([0, EMPTY]))
        assert known.cpu().tolist() == [1, 1]
    store.close()


@pytest.mark.parametrize("how", ["add", "add_index"])
@pytest.mark.parametrize("skip", [True, False])
def test_store_grows_with_all_ones_held(gpu, skip, how):
    c = K.grow(skip)
    calls = [np.array([EMPTY, 0, EMPTY], np.uint64)] + c.calls[:-1] + [c.calls[-1][:-3]]  # (4096 hashes in all: 8192 slots at the end)
    sizes = table_sizes(0, [len(x) for x in calls])
    assert sizes[-1][0] == 8192 and sizes[-1][1] >= 3
    store = Store(gpu, 0)
    pos, allh = 0, np.concatenate(calls)
    for x, (slots, grown) in zip(calls, sizes):
        store.add(dev(x)) if how == "add" else store.add_index(chunk_index_of(x))
        pos += len(x)
        assert store.added == pos and store.grown == grown and store.distinct == len(np.unique(allh[:pos]))
        check_finds(store, allh[:pos], slots)
        known, count = store.find(dev([EMPTY, 0, K.key_at(0, K.FAR)]))
        assert known.cpu().tolist() == [1, 1, 0] and int(count.item()) == 2
    store.close()


def test_store_distinct_counts_a_lone_claim(gpu):
    c = K.lone_claim()
    store = Store(gpu, 0)
    for i, x in enumerate(c.calls):
        store.add(dev(x))
        assert store.distinct == i + 1, c.notes["subs"][i - 1] if i else "the first key"
    known, count = store.find(dev(np.unique(c.hashes)))
    assert known.cpu().numpy().all() and int(count.item()) == len(c.calls)
    store.close()


# ---- the second table: lthip_get_existing_store_index -----------------------------------------------------------------------------------


@pytest.mark.parametrize("percent", [0, 1, 50, 100])
@pytest.mark.parametrize("wanted", ["all", "all-ones not wanted", "all-ones alone"])
def test_existing_store_index_is_the_references_bytes(gpu, ref, wanted, percent):
    blocks, sets = K.store_index_inputs()
    blob, w = K.store_index_blob(blocks), sets[wanted]
    expect = ref.get_existing_store_index(blob, w, percent)
    taken = K.store_index_hashes(expect)[0].tolist()
    a, b, c = (blocks[i][0] for i in range(3))
    if percent <= 50:  # (what the blocks are there for, read off the reference's own answer)
        assert {"all": a in taken and b not in taken and c in taken,
                "all-ones not wanted": b not in taken and (c in taken) == (percent < 50),  # (C is then a quarter wanted, not a half)
                "all-ones alone": taken == ([b] if percent < 50 else [])}[wanted]
    assert gpu.get_existing_store_index(blob, dev(w), percent) == expect


# ---- lthip_create_missing_content on the one-shot table ---------------------------------------------------------------------------------


def gpu_missing_content(gpu, inp):
    return gpu.create_missing_content(dev(inp["existing"]), dev(inp["hashes"]), dev32(inp["sizes"]), inp["tags"], inp["max_block_size"],
                                      inp["max_chunks_per_block"])


@pytest.mark.parametrize("where", K.MISSING_WHERE)
@pytest.mark.parametrize("kind", K.MISSING_KINDS)
def test_missing_content_is_the_references_bytes(gpu, ref, kind, where):
    """Store and version fill the 1024 slots to the half with one cluster; the version's chunk list is unique, as a VersionIndex's is."""
    inp = K.missing_content_inputs(kind, where, repeats=False)
    assert gpu_missing_content(gpu, inp) == K.ref_missing_content(ref, inp)


@pytest.mark.parametrize("where", K.MISSING_WHERE)
@pytest.mark.parametrize("kind", K.MISSING_KINDS)
def test_missing_content_of_a_version_with_repeats_is_the_references_bytes(gpu, ref, kind, where):
    """A version list with repeats, of keys the store holds and of keys it lacks, is outside the contract of the call and of the
    reference; the reference's answer to one (tests/test_hash_table_keys_cases.py::test_what_the_reference_makes_of_a_list_with_repeats:
    it leaves out 18 to 22 of the about 300 chunks these stores lack) is the device call's, byte for byte."""
    inp = K.missing_content_inputs(kind, where)
    assert len(np.unique(inp["hashes"])) < len(inp["hashes"]) and len(inp["existing"]) + len(inp["hashes"]) == 512
    assert gpu_missing_content(gpu, inp) == K.ref_missing_content(ref, inp)


def test_missing_content_of_lists_that_are_mostly_repeats_is_the_references_bytes(gpu, ref):
    """Short lists drawn from fewer hashes than they have entries: the reference's walk meets entries twice, fills the list of added
    hashes before its end, or leaves sorted hashes behind it."""
    for inp in K.mostly_repeats_inputs():
        assert gpu_missing_content(gpu, inp) == K.ref_missing_content(ref, inp), (inp["existing"], inp["hashes"])
