"""The parts of tests/buzhash_rot_table.py proved on the CPU, before tests/test_gpu_buzhash_rot_table.py sends them through the scans:
  - part A holds every (byte value, position mod 32) pair at least 8 times, parts B only the eight values of one LDS bank, part C one
    byte around 4 KiB of random ones;
  - a numpy model of a scan that reads U[q] from the 32 x 256 table of rotations gives the oracle's chunks on every part;
  - with ONE entry of the table wrong -- the corners r = 0, r = 31, v = 0, v = 255 among them -- the model cuts part A differently, for a
    discriminator that is a power of two and for one that is not: the chunk list of part A depends on every entry tried (no kernel is
    ever run broken)."""
import numpy as np
import pytest

from tests import buzhash_plants as P
from tests import buzhash_rot_table as R


def test_the_parts_are_what_they_claim():
    parts = R.parts()
    assert {k: len(v) for k, v in parts.items()} == {"A": 256 << 10, "B0": 64 << 10, "B31": 64 << 10, "C": 64 << 10}
    n = R.pair_counts(parts["A"])
    print("part A: (byte, position mod 32) pairs occur", int(n.min()), "to", int(n.max()), "times")
    assert n.min() >= 8
    for c in (0, 31):
        vals = np.unique(parts[f"B{c}"])
        assert vals.tolist() == [c + 32 * k for k in range(8)] and set(int(v) % 32 for v in vals) == {c}  # one bank, all eight of its values
        assert (R.pair_counts(parts[f"B{c}"])[:, vals] > 0).all()  # each of them at every rotation
    c = parts["C"]
    assert (c[: 30 << 10] == 0xA7).all() and (c[34 << 10 :] == 0xA7).all() and len(np.unique(c[30 << 10 : 34 << 10])) == 256
    assert [P.disc(av) for _, av, _ in R.CFGS + [R.HEADLINE]] == [96, 64, 24680]


def test_the_table_of_rotations():
    t = R.rot_table()
    assert t.shape == (32, 256) and t.dtype == np.uint32 and (t[0] == P.TABLE).all()
    for r in (1, 16, 31):
        assert all(P._rotl(int(t[r][v]), r) == int(P.TABLE[v]) for v in (0, 1, 128, 255))


@pytest.mark.parametrize("cfg", R.CFGS + [R.HEADLINE])
def test_model_agrees_with_the_oracle(oracle, cfg):
    t = R.rot_table()
    for name, a in R.parts().items():
        _, e_len, _ = oracle.chunk_and_hash(a, *cfg)
        got = R.model_lengths(a, cfg, t)
        assert len(got) == len(e_len) and (got == e_len).all(), (name, cfg)
        assert (P.model_lengths(a, cfg) == e_len).all(), (name, cfg)  # (and the model of tests/buzhash_plants.py, which rotates T itself)
    # the parts cut by candidates, not only at max: the cut test sees the hashes
    a_len = oracle.chunk_and_hash(R.parts()["A"], *cfg)[1]
    assert np.count_nonzero(a_len < cfg[2]) >= (1000 if cfg != R.HEADLINE else 5)


def corruptions():
    """(r, v, xor): the four corners in every pairing, then seeded ones -- 72 single entries."""
    rng = np.random.default_rng(R.SEED + 1)
    out = [(r, v, 1 << b) for r in (0, 31) for v in (0, 255) for b in (0, 31)]
    out += [(0, int(rng.integers(256)), 0x00010000), (31, int(rng.integers(256)), 0x00000100), (int(rng.integers(32)), 0, 0x01000000),
            (int(rng.integers(32)), 255, 0x00000010)]
    while len(out) < 72:
        out.append((int(rng.integers(32)), int(rng.integers(256)), int(rng.integers(1, 1 << 32))))
    return out


@pytest.mark.parametrize("cfg", R.CFGS)
def test_every_corrupted_entry_changes_part_a(cfg):
    a, good = R.parts()["A"], R.rot_table()
    want = R.model_lengths(a, cfg, good)
    cases = corruptions()
    assert len(cases) >= 64 and len(set((r, v) for r, v, _ in cases)) >= 64
    unseen = []
    for r, v, x in cases:
        bad = good.copy()
        bad[r][v] ^= np.uint32(x)
        got = R.model_lengths(a, cfg, bad)
        if len(got) == len(want) and (got == want).all():
            unseen.append((r, v, hex(x)))
    assert not unseen, (cfg, unseen)
