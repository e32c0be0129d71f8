"""bench.py --dump-outputs without a GPU: dump_outputs on host tensors standing in for the session's buffers -- float files only,
within the 64 MB bound, the same sample for the same sizes, and every value traceable to the array it was taken from."""
import types

import numpy as np
import torch

import bench


def fake_session(seed, n=300000):
    rng = np.random.default_rng(seed)
    t = dict(hash=torch.from_numpy(rng.integers(0, 2**63, n, dtype=np.int64)),
             lens=torch.from_numpy(rng.integers(1, 1 << 17, n).astype(np.int32)),
             arena=torch.from_numpy(rng.integers(0, 256, 40 << 20, dtype=np.uint8)),
             vi=torch.from_numpy(rng.integers(0, 256, 4 << 20, dtype=np.uint8)), si=torch.from_numpy(rng.integers(0, 256, 4096, dtype=np.uint8)))
    t["offs"] = torch.from_numpy(np.cumsum(t["lens"].numpy().astype(np.int64)))
    img_off, img_size = np.array([0, 10 << 20, 11 << 20], np.uint64), np.array([5 << 20, 3, 20 << 20], np.uint32)
    ing = types.SimpleNamespace(images=lambda: (7, img_off, img_size))
    res = types.SimpleNamespace(chunks_all=n, unique_all=n, blocks=3, raw_bytes=1, compressed_bytes=2, version_index_size=3 << 20,
                                store_index_size=1000)
    args = (ing, res, n, t["offs"], t["lens"], t["hash"], np.array([0, 5, n], np.uint32), t["vi"], t["si"], np.array([9, 8, 7], np.uint32), t["arena"])
    return t, (img_off, img_size), args


def test_dump_outputs_are_float_bounded_and_traceable(tmp_path):
    t, (img_off, img_size), args = fake_session(0)
    names = bench.dump_outputs(tmp_path / "a", *args)
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    idx = got["chunk_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE and (np.diff(idx) > 0).all()
    h = got["chunk_hashes"].astype(np.uint64)
    assert ((h[:, 0] | (h[:, 1] << np.uint64(32))) == t["hash"].numpy().view(np.uint64)[idx]).all()
    assert (got["chunk_lengths"] == t["lens"].numpy()[idx]).all() and (got["chunk_offsets"] == t["offs"].numpy()[idx]).all()
    i = got["version_index_bytes_index"].astype(np.int64)
    assert i.max() < 3 << 20 and (got["version_index_bytes"] == t["vi"].numpy()[i]).all()
    assert (got["store_index_bytes"] == t["si"].numpy()[:1000]).all()
    laid = np.concatenate([t["arena"].numpy()[int(o) : int(o) + int(s)] for o, s in zip(img_off, img_size)])
    assert (got["image_bytes"] == laid[got["image_bytes_index"].astype(np.int64)]).all()
    # the same sizes give the same sample: two runs of one build compare position for position
    _, _, other = fake_session(1)
    again = bench.dump_outputs(tmp_path / "b", *other)
    assert again == names
    for k in ("chunk_index", "version_index_bytes_index", "image_bytes_index"):
        assert (np.load(tmp_path / "b" / f"{k}.npy") == got[k]).all()
