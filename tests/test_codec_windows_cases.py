"""The case tables and layouts of tests/codec_windows_util.py, checked on the CPU with the oracle (and the reference where it is built):
every "valid" LZ4 payload is accepted with its size, every "wants more room" payload is rejected, every class the GPU test names has
a case, and the two layouts are what they claim to be.  With this, a failure of tests/test_gpu_codec_windows.py is the kernels'."""
import numpy as np
import pytest

from tests import codec_windows_util as W
from tests._libs import have_ref, ref as get_ref


@pytest.mark.parametrize("content", W.LZ4_DEC_CONTENTS)
def test_valid_lz4_payloads_are_accepted_with_their_size(oracle, content):
    pairs = W.lz4_valid_payloads(oracle, content)
    assert [len(r) for r, _ in pairs] == W.LZ4_DEC_SIZES
    for raw, p in pairs:
        n, out = oracle.lz4_decompress(p, len(raw))
        assert n == len(raw) and (out == raw).all()
        if have_ref():
            err, out2 = get_ref().decompress(0, p, len(raw))
            assert err == 0 and len(out2) == len(raw) and (out2 == raw).all()
        if content == "noise":
            assert len(p) == W.lz4_literal_run_size(len(raw))  # one literal run
        if content == "zeros" and len(raw) >= 2047:
            assert len(p) < 16 + len(raw) // 250  # one match: a token, its length bytes, the last literals
    cases = W.lz4_valid_cases(oracle, content)
    assert len(cases) == len(W.LZ4_DEC_SIZES) * 16 * len(W.LZ4_DEC_SRC_RES)
    assert {(s, d) for _, _, s, d in cases} == {(s, d) for s in W.LZ4_DEC_SRC_RES for d in range(16)}


def test_lz4_payloads_that_want_more_room_are_rejected(oracle):
    cases = W.lz4_overshoot_cases(oracle)
    big = [n for n in W.LZ4_DEC_SIZES if n >= 16]
    assert len(cases) == len(big) * len(W.LZ4_OVERSHOOTS) * len(W.LZ4_TAILS)
    seen = set()
    for c in cases:
        n, _ = oracle.lz4_decompress(c["payload"], c["cap"])
        assert n < 0, (c["cap"], c["k"], c["tail"])
        full, _ = oracle.lz4_decompress(c["payload"], c["cap"] + c["k"])
        assert full == c["cap"] + c["k"]  # it is the room alone that is missing
        if have_ref():
            err, _ = get_ref().decompress(0, c["payload"], c["cap"])
            assert err != 0
        seen.add((c["cap"], c["k"], c["tail"]))
    assert seen == {(n, k, t) for n in big for k in W.LZ4_OVERSHOOTS for t in W.LZ4_TAILS}
    assert {c["dres"] for c in cases} == set(range(16)) and {c["sres"] for c in cases} == set(W.LZ4_DEC_SRC_RES)
    assert any(c["cap"] >= 131072 for c in cases) and any(c["cap"] < 131072 for c in cases)  # both decoders


def test_damaged_lz4_payloads_have_both_verdicts(oracle):
    cases = W.lz4_fuzz_cases(oracle)
    verdicts = [oracle.lz4_decompress(c, cap)[0] >= 0 for c, cap in cases]
    assert len(cases) == 8 * 25 and 8 <= sum(verdicts) < len(cases)
    raws = W.lz4_pd_fuzz_raws(oracle)
    cases = W.lz4_pd_fuzz_cases(oracle, raws, [oracle.lz4_compress(r) for r in raws])  # (the oracle's payloads stand in for the HIP encoder's)
    assert len(cases) == 5 * 2 * 17 and all(cap >= 131072 for _, cap in cases)  # the block-parallel decoder's
    assert any(oracle.lz4_decompress(c, cap)[0] < 0 for c, cap in cases)


def test_encoder_and_zstd_tables_hold_every_class(oracle):
    lz = W.enc_cases(oracle, W.LZ4_ENC_SIZES, W.LZ4_ENC_KINDS)
    assert len(lz) == len(W.LZ4_ENC_SIZES) * 3 * 4 * 16
    assert {(len(r), k, s, d) for r, s, d, k in lz} == {(n, k, s, d) for n in W.LZ4_ENC_SIZES for k in W.LZ4_ENC_KINDS
                                                        for s in W.ENC_SRC_RES for d in range(16)}
    zs = W.enc_cases(oracle, W.ZSTD_ENC_SIZES, W.ZSTD_ENC_KINDS)
    assert len(zs) == len(W.ZSTD_ENC_SIZES) * 4 * 4 * 16
    assert [len(r) for r in W.zstd_raws(oracle)] == W.ZSTD_DEC_SIZES * len(W.ZSTD_KINDS)
    assert W.ZSTD_CHAIN_SIZE < int(1.3 * (1 << 20)) and (W.ZSTD_CHAIN_SIZE + 131071) // 131072 == 10
    # a noise block is one literal run, and the cut capacities end inside its first, second and sixteenth 4 KiB unit
    for n in (4095, 65536, 200000):
        noise = W.zstd_raw(oracle, n, 0)
        assert len(oracle.lz4_compress(noise)) == W.lz4_literal_run_size(n)
        caps = W.lz4_noise_cut_caps(n)
        head = W.lz4_literal_run_size(n) - n
        assert sorted({(c - head) // 4096 for c in caps}) == [0, 1, 15] and {(c - head) % 4096 for c in caps} == {0, 1, 4095}
    assert W.zstd_trailer_size(1) == 14 and W.zstd_trailer_size(4097) == 16 and W.zstd_trailer_size(400000) == 12 + 2 * 98


def test_zstd_damaged_frames_are_the_existing_tests(oracle, ref):
    cases = W.zstd_damaged_frames(oracle, ref)
    assert len(cases) == 5 * 2 * 60 and any(cap < 3000 for _, cap in cases)


@pytest.mark.parametrize("mode", ["guarded", "packed"])
def test_layouts(mode):
    rng = np.random.default_rng(5)
    specs = [(s, d, cap) for s in (0, 1, 5, 15) for d in range(16) for cap in (0, 1, 15, 16, 17, 100, 4097)]
    blocks = [rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8) for _ in specs]
    lay = W.build_layout(blocks, specs, mode)
    assert lay.dst_len % 16 == 0 and len(lay.src) % 16 == 0 and len(lay.outside) == lay.dst_len
    for b, (blk, (s, d, cap)) in enumerate(zip(blocks, specs)):
        so, do = lay.src_offs[b], lay.dst_offs[b]
        assert so % 16 == s and (lay.src[so : so + len(blk)] == blk).all() and lay.src_sizes[b] == len(blk) and lay.caps[b] == cap
        assert not lay.outside[do : do + cap].any()
        prev_end = lay.dst_offs[b - 1] + lay.caps[b - 1] if b else 0
        if mode == "guarded":
            assert do % 16 == d and do - prev_end >= W.GUARD and lay.outside[do - W.GUARD : do].all()
            assert lay.outside[do + cap : do + cap + W.GUARD].all() and do + cap + W.GUARD <= lay.dst_len
        else:
            assert do == (prev_end if b else W.END_GUARD)  # no gap at all
    last = lay.dst_offs[-1] + lay.caps[-1]
    end = W.GUARD if mode == "guarded" else W.END_GUARD
    assert lay.dst_len - last >= end and lay.outside[last:].all() and lay.outside[: lay.dst_offs[0]].all() and lay.dst_offs[0] >= end
    assert int(lay.outside.sum()) == lay.dst_len - sum(lay.caps)
    # the two fills differ in every byte, and neither is a constant
    p = W.pattern(4096)
    assert ((p ^ ~p) == 0xFF).all() and len(np.unique(p)) > 200
    # a stray byte is blamed on the nearest window
    if mode == "guarded":
        assert "3 bytes in front of the window of block 37 " in lay.blame(lay.dst_offs[37] - 3)
    assert f"1 bytes past the end of the window of block {len(specs) - 1} " in lay.blame(last)
