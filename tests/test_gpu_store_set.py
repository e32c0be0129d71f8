"""-m gpu: lthip_store, the device-resident set of the chunk hashes a store already holds (k_dedup.hip).  Its defining property:
whatever way the hashes were added -- one call, many, through a StoreIndex blob, with the table grown from its smallest size or never
grown -- lthip_store_find answers numpy's isin, and counts its ones.  The hashes 0 and 0xFFFF...FFFF (the table's empty key) are
members like any other; a malformed StoreIndex and a failed growth change nothing."""
import errno

import numpy as np
import pytest
import torch

from longtail_amd.lib import LongtailHipError, Seen, Store

pytestmark = pytest.mark.gpu

DISTINCT, N, QUERIES = 3_000, 8_000, 20_001
EMPTY = 0xFFFFFFFFFFFFFFFF


def dev(h):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def hashes():
    """(what is added: all DISTINCT hashes of the pool, with repeats, N in all; the queries: half drawn from the pool, half not)"""
    rng = np.random.default_rng(17)
    pool = np.unique(rng.integers(1, 2**64 - 1, size=DISTINCT + 64, dtype=np.uint64))[:DISTINCT]
    pool = pool[rng.permutation(DISTINCT)]
    added = np.concatenate([pool, pool[rng.integers(0, DISTINCT, size=N - DISTINCT)]])[rng.permutation(N)]
    assert len(np.unique(added)) == DISTINCT
    inside = pool[rng.integers(0, DISTINCT, size=QUERIES // 2)]
    outside = rng.integers(1, 2**64 - 1, size=QUERIES - QUERIES // 2, dtype=np.uint64)
    queries = np.concatenate([inside, outside])[rng.permutation(QUERIES)]
    return added, queries


def cuts_of(kind):
    if kind == "one":
        return [N]
    if kind == "ones-then-rest":
        return [1] * 64 + [N - 64]
    rng = np.random.default_rng(5)
    sizes = []
    while sum(sizes) < N:
        sizes.append(min(int(rng.integers(0, 701)) if len(sizes) % 7 else 0, N - sum(sizes)))
    assert 0 in sizes and len(sizes) > 20
    return sizes


@pytest.mark.parametrize("expected", [0, N])
@pytest.mark.parametrize("kind", ["one", "ones-then-rest", "random"])
def test_membership_is_isin_whatever_the_cutting(gpu, hashes, kind, expected):
    added, queries = hashes
    store = Store(gpu, expected)
    pos = 0
    for k in cuts_of(kind):
        assert store.added == pos
        store.add(dev(added[pos : pos + k]))
        pos += k
    assert store.added == N and store.distinct == DISTINCT
    # 1024 slots hold 512 hashes: a store made for none has grown; one made for N (two slots per hash ADDED, repeats included) has not
    assert (store.grown >= 1) if expected == 0 else (store.grown == 0)
    want = np.isin(queries, added)
    assert 0.45 * QUERIES < want.sum() < 0.55 * QUERIES
    for n in (QUERIES, 0, 1, 63, 64, 65):  # (the edges of the per-wave count)
        q = dev(queries[:n])
        known, count = store.find(q)
        assert (known.cpu().numpy() == want[:n]).all(), n
        assert int(count.item()) == int(want[:n].sum()) == int(known.sum().item()), n
        store.find(q, count=count)  # the counter is set by the call, not added to
        assert int(count.item()) == int(want[:n].sum()), n
    store.close()


def test_the_two_special_values(gpu):
    both = np.array([0, EMPTY], np.uint64)
    rng = np.random.default_rng(2)
    others = rng.integers(1, 2**64 - 1, size=700, dtype=np.uint64)  # (more than 512: the table grows with the flag set)
    holds, lacks, never = Store(gpu, 0), Store(gpu, 0), Store(gpu, 0)
    holds.add(dev(both))
    holds.add(dev(both[::-1].copy()))
    holds.add(dev(others))
    lacks.add(dev(others))
    q = np.concatenate([both, others[:5], np.array([12345], np.uint64)])
    for store, want in ((holds, [1, 1, 1, 1, 1, 1, 1, 0]), (lacks, [0, 0, 1, 1, 1, 1, 1, 0]), (never, [0] * 8)):
        known, count = store.find(dev(q))
        assert known.cpu().tolist() == want and int(count.item()) == sum(want)
    assert holds.distinct == 702 and lacks.distinct == 700 and never.distinct == 0
    assert holds.grown >= 1 and never.grown == 0 and never.added == 0
    for s in (holds, lacks, never):
        s.close()


def test_add_index_adds_the_chunk_hashes_of_a_store_index(gpu, hashes):
    added, queries = hashes
    uniq = added[np.sort(np.unique(added, return_index=True)[1])]
    lens = (np.arange(len(uniq)) % 5000 + 100).astype(np.uint32)
    blob = gpu.create_missing_content(None, dev(uniq), torch.from_numpy(lens.view(np.int32)).cuda(), None, 65536, 64)
    head = np.frombuffer(blob[:16], np.uint32)
    nb, m = int(head[2]), int(head[3])
    assert m == DISTINCT and nb > 1
    by_index, by_add = Store(gpu, 0), Store(gpu, 0)
    by_add.add(dev(uniq))
    part = dev(uniq[:10])
    by_index.add(part)
    want_small = np.isin(queries, uniq[:10])
    # ---- a blob cut inside its header, one cut in the middle of the chunk-hash array, one of another version: EBADF, nothing changed ----
    other_version = bytearray(blob)
    other_version[3] = 2
    for bad in (blob[:15], blob[: 16 + nb * 8 + (m // 2) * 8 + 3], bytes(other_version)):
        with pytest.raises(LongtailHipError) as e:
            by_index.add_index(bad)
        assert e.value.code == errno.EBADF
        assert by_index.added == 10 and by_index.distinct == 10 and by_index.grown == 0
        known, count = by_index.find(dev(queries))
        assert (known.cpu().numpy() == want_small).all() and int(count.item()) == int(want_small.sum())
    # ---- the whole blob: the same set as add() of its chunk hashes ----
    by_index.add_index(blob)
    assert by_index.added == 10 + DISTINCT and by_index.distinct == DISTINCT == by_add.distinct and by_index.grown >= 1
    k1, c1 = by_index.find(dev(queries))
    k2, c2 = by_add.find(dev(queries))
    assert (k1 == k2).all() and int(c1.item()) == int(c2.item()) == int(np.isin(queries, uniq).sum())
    by_index.add_index(np.array([1 << 24, 0, 0, 0], np.uint32).tobytes())  # an index without chunks adds nothing
    assert by_index.added == 10 + DISTINCT
    by_index.close()
    by_add.close()


def test_two_stores_a_seen_table_and_a_one_shot_call_do_not_disturb_each_other(gpu):
    rng = np.random.default_rng(3)
    arrays = [rng.integers(0, 500 * (k + 1), size=6_000, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) for k in range(4)]
    queries = np.concatenate([a[::7] for a in arrays])
    a, b, seen = Store(gpu, 0), Store(gpu, 0), Seen(gpu, 0)
    firsts, third, answers = [], None, []
    for i in range(0, 6_000, 750):
        a.add(dev(arrays[0][i : i + 750]))
        firsts.append(seen.add(dev(arrays[2][i : i + 750]))[0])
        if i == 2_250:
            third = gpu.dedup_first_seen(dev(arrays[3]))
            answers.append((a.find(dev(queries))[0], b.find(dev(queries))[0], i + 750))
        b.add(dev(arrays[1][i : i + 750]))
    gpu.sync()

    def first_occurrence(h):
        _, first, inverse = np.unique(h, return_index=True, return_inverse=True)
        return first[inverse].astype(np.int64)

    for ka, kb, n in answers:  # (in the middle: a holds n of its hashes, b those of the calls before this one)
        assert (ka.cpu().numpy() == np.isin(queries, arrays[0][:n])).all() and (kb.cpu().numpy() == np.isin(queries, arrays[1][: n - 750])).all()
    assert (a.find(dev(queries))[0].cpu().numpy() == np.isin(queries, arrays[0])).all()
    assert (b.find(dev(queries))[0].cpu().numpy() == np.isin(queries, arrays[1])).all()
    assert (torch.cat(firsts).cpu().numpy().astype(np.int64) == first_occurrence(arrays[2])).all()
    assert (third[0].cpu().numpy().astype(np.int64) == first_occurrence(arrays[3])).all()
    assert a.grown > 0 and b.grown > 0 and seen.grown > 0
    assert a.distinct == len(np.unique(arrays[0])) and b.distinct == len(np.unique(arrays[1]))
    for t in (a, b, seen):
        t.close()


def test_an_allocation_failing_while_the_table_grows_is_enomem_and_changes_nothing(gpu_abl):
    """lthip_debug_fail_alloc of the ablation build (an errno from the library's allocator, no device fault): the add that has to grow
    the table returns ENOMEM, the old table stays live with its answers, and the next add grows and succeeds."""
    d = gpu_abl.lib.dll
    assert d.lthip_debug_fail_alloc(-1, 0) == 0, "the ablation build must have the injection switch"
    rng = np.random.default_rng(9)
    h = np.unique(rng.integers(1, 2**64 - 1, size=2_100, dtype=np.uint64))[:2_000]
    q = np.concatenate([h[::3], rng.integers(1, 2**64 - 1, size=500, dtype=np.uint64)])
    store = Store(gpu_abl, 0)
    try:
        store.add(dev(h[:400]))  # 800 of 1024 slots' worth: no growth
        assert store.grown == 0 and store.distinct == 400
        before = store.find(dev(q))[0].cpu().numpy()
        assert (before == np.isin(q, h[:400])).all()
        d.lthip_debug_fail_alloc(0, 1)
        try:
            with pytest.raises(LongtailHipError) as e:
                store.add(dev(h[400:]))
        finally:
            d.lthip_debug_fail_alloc(-1, 0)
        assert e.value.code == errno.ENOMEM
        assert store.added == 400 and store.grown == 0 and store.distinct == 400
        assert (store.find(dev(q))[0].cpu().numpy() == before).all()
        store.add(dev(h[400:]))
        assert store.added == 2_000 and store.grown == 1 and store.distinct == 2_000
        known, count = store.find(dev(q))
        assert (known.cpu().numpy() == np.isin(q, h)).all() and int(count.item()) == int(np.isin(q, h).sum())
    finally:
        d.lthip_debug_fail_alloc(-1, 0)
        store.close()
