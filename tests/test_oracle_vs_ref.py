"""Fuzz the oracle against the reference library itself: live where oracle/_ref was built, elsewhere against the reference's
results recorded under tests/golden/ref_results.json (the `refcall` fixture).  CPU only."""
import numpy as np
import pytest

from tests._libs import digest


def test_blake3_fuzz(oracle, refcall):
    rng = np.random.default_rng(3)
    buf = rng.integers(0, 256, size=400000, dtype=np.uint8)
    pieces = []
    for _ in range(300):
        n = int(rng.choice([rng.integers(0, 200), rng.integers(0, 5000), rng.integers(0, 400000)]))
        s = int(rng.integers(0, len(buf) - n + 1))
        pieces.append(buf[s : s + n])
    want = refcall("blake3", pieces, lambda r: [r.blake3(p) for p in pieces])
    assert [oracle.blake3(p) for p in pieces] == want


@pytest.mark.parametrize("cfg", [(8192, 32768, 131072), (48, 48, 48), (4096, 16384, 65536), (48, 100, 300), (16384, 65536, 262144), (48, 64, 64)])
def test_chunker_fuzz(oracle, refcall, cfg):
    rng = np.random.default_rng(cfg[0])
    for kind in (0, 1, 2):
        size = int(rng.integers(1, 6 << 20))
        data = oracle.synth(size, 1000 + kind, kind)
        o_offs, o_lens, o_hashes = oracle.chunk_and_hash(data, *cfg)
        r_offs, r_lens, r_hashes = refcall("chunk_and_hash", [data, cfg], lambda r: [digest(a) for a in r.chunk_and_hash(data, *cfg)])
        assert digest(o_lens) == r_lens and digest(o_hashes) == r_hashes and digest(o_offs) == r_offs
        assert digest(oracle.chunk(data, *cfg, pure=True)) == r_lens


def test_chunker_edge_sizes(oracle, refcall):
    cfg = (8192, 32768, 131072)
    base = oracle.synth(400000, 77, 0)
    for size in [0, 1, 47, 48, 49, 8191, 8192, 8193, 131071, 131072, 131073, 262144, 262145]:
        d = base[:size].copy()
        want = refcall("chunk_and_hash.lens", [d, cfg], lambda r: r.chunk_and_hash(d, *cfg)[1].tolist())
        assert oracle.chunk(d, *cfg).tolist() == want, size


def test_from_buffer_differs_from_stream_somewhere(oracle, refcall):
    # the two entry points are NOT equivalent; the restatement must follow each one
    cfg = (8192, 32768, 131072)
    found = False
    for seed in range(40):
        d = oracle.synth(8 << 20, 500 + seed, 0)
        fb = refcall("chunk_from_buffer", [d, cfg], lambda r: r.chunk_from_buffer(d, *cfg).tolist())
        st = refcall("chunk_and_hash.lens", [d, cfg], lambda r: r.chunk_and_hash(d, *cfg)[1].tolist())
        pos, mine = 0, []
        while pos < len(d):
            n = int(oracle.dll.lto_hpcdc_next_from_buffer(d[pos:].ctypes.data, len(d) - pos, *cfg))
            mine.append(n)
            pos += n
        assert mine == list(fb)
        if list(fb) != list(st):
            found = True
            break
    assert found, "expected at least one stream where NextChunkFromBuffer diverges from NextChunk"


def decoded(r, codec, comp, cap):
    """the reference decoder's answer, small: [error, length, digest of the bytes]"""
    err, out = r.decompress(codec, comp, cap)
    return [int(err), len(out), digest(out)]


def test_lz4_fuzz(oracle, refcall):
    rng = np.random.default_rng(11)
    for kind in (0, 1, 2):
        for n in [0, 1, 12, 13, 64, 4096, 65546, 65547, 200000, (1 << 20) + 7]:
            d = oracle.synth(n, 90 + n, kind)
            a = refcall("lz4_compress", [d], lambda r: digest(r.compress(0, r.lz4_type, d)))
            b = oracle.lz4_compress(d)
            assert a == digest(b), (kind, n)
            assert refcall("lz4_decompress", [b, n], lambda r: decoded(r, 0, b, n)) == [0, n, digest(d)]
    # decoders agree on corrupted streams (c: the reference's payload, the restatement's bytes as asserted above)
    d = oracle.synth(6000, 3, 1)
    c = oracle.lz4_compress(d)
    assert refcall("lz4_compress", [d], lambda r: digest(r.compress(0, r.lz4_type, d))) == digest(c)
    accepted = []
    for _ in range(1500):
        c2 = c.copy()
        c2[rng.integers(0, len(c2))] = rng.integers(0, 256)
        if rng.random() < 0.3:
            c2 = c2[: rng.integers(1, len(c2))].copy()
        k, _o = oracle.lz4_decompress(c2, 6000)
        if k >= 0:
            accepted.append((c2, [0, int(k), digest(_o)]))
    # the restatement applies the strict end-of-block rules on every path (the reference's shortcut paths let
    # some malformed streams through): whatever it accepts the reference accepts, with identical output
    streams = [c2 for c2, _ in accepted]
    want = refcall("lz4_decompress_many", streams + [6000], lambda r: [decoded(r, 0, c2, 6000) for c2 in streams])
    assert want == [mine for _, mine in accepted]
