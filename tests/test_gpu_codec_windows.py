"""-m gpu: the four block codec calls never write outside a block's destination window (the contract in longtail_hip.h).  Every call is
made on the guarded and the packed layout of tests/codec_windows_util.py, twice (a position-dependent fill and its complement); the
sizes and bytes a call must give come from the oracle, the reference and the source data, and no byte outside the union of the windows
may change -- for valid payloads at every alignment and at the sizes where the decoders change paths, for payloads that want more room
than they get, for damaged payloads, and for encoders whose capacity ends at each edge of what they place speculatively.
tests/test_codec_windows_cases.py checks the case tables themselves on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import codec_windows_util as W
from tests._libs import have_ref, ref as get_ref

pytestmark = pytest.mark.gpu

MODES = ["guarded", "packed"]


def check(lay, results, expect):
    """guards, then per block: expect[b] is None (the call must refuse the block: 0xFFFFFFFF from a decoder), 0 (an encoder's "does not
    fit") or the bytes the window must begin with"""
    W.check_guards(lay, results)
    want = np.array([W.REFUSED if e is None else 0 if isinstance(e, int) else len(e) for e in expect], np.uint32)
    for res in results:
        bad = np.flatnonzero(res.sizes != want)
        assert bad.size == 0, f"{bad.size} sizes differ, the first: {int(res.sizes[bad[0]])} for {int(want[bad[0]])}, {lay.describe(int(bad[0]))}"
        for b, e in enumerate(expect):
            if e is not None and not isinstance(e, int):
                assert (res.windows[b][: len(e)] == e).all(), f"bytes differ, {lay.describe(b)}"


def encode(call, raws, bound):
    """the library's own payloads of `raws` (inputs of decoder tests), from aligned guarded windows of the codec's bound"""
    lay = W.build_layout(raws, [(0, 0, bound(len(r))) for r in raws], "guarded")
    results = W.run(lay, call)
    W.check_guards(lay, results)
    return [w[: int(s)].copy() for w, s in zip(results[0].windows, results[0].sizes)]


# ---- LZ4 decode ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("content", W.LZ4_DEC_CONTENTS)
def test_lz4_decode_valid_payloads_stay_in_their_windows(gpu, oracle, mode, content):
    """16 destination residues x 6 source residues x 21 sizes around the flush granule, the ring, the direct long-literal path, the unit
    and the block-parallel threshold: the oracle's payloads decode to the raws and nothing lands beside a window."""
    cases = W.lz4_valid_cases(oracle, content)
    lay = W.build_layout([p for _, p, _, _ in cases], [(s, d, len(r)) for r, _, s, d in cases], mode)
    check(lay, W.run(lay, gpu.lz4_decompress_blocks), [r for r, _, _, _ in cases])


@pytest.mark.parametrize("mode", MODES)
def test_lz4_decode_refuses_payloads_that_want_more_room(gpu, oracle, mode):
    """A payload of n + k bytes in a window of n: refused, nothing past the window -- with the final literal run, the last match, or the
    match and then the last five literals crossing the end.  Packed: a valid block lies on either side of each and decodes exactly."""
    blocks, specs, expect = [], [], []
    near = [(r, oracle.lz4_compress(r)) for r in (oracle.synth(100, 7, 1), np.zeros(2049, np.uint8), oracle.synth(17, 8, 0))]
    for i, c in enumerate(W.lz4_overshoot_cases(oracle)):
        if mode == "packed":
            r, p = near[i % 3]
            blocks.append(p), specs.append((i % 16, 0, len(r))), expect.append(r)
        blocks.append(c["payload"]), specs.append((c["sres"], c["dres"], c["cap"])), expect.append(None)
    if mode == "packed":
        blocks.append(near[0][1]), specs.append((0, 0, len(near[0][0]))), expect.append(near[0][0])
    lay = W.build_layout(blocks, specs, mode)
    check(lay, W.run(lay, gpu.lz4_decompress_blocks), expect)


def _damaged_lz4(gpu, oracle, cases):
    lay = W.build_layout([c for c, _ in cases], [(i % 16, 1 + i % 15, cap) for i, (_, cap) in enumerate(cases)], "guarded")
    expect = []
    for c, cap in cases:
        n, out = oracle.lz4_decompress(c, cap)
        expect.append(None if n < 0 else out[:n])
    check(lay, W.run(lay, gpu.lz4_decompress_blocks), expect)
    assert any(e is None for e in expect) and any(e is not None for e in expect)


def test_lz4_decode_damaged_payloads_stay_in_their_windows(gpu, oracle):
    """the damaged payloads of test_lz4_gpu_decoder_differential_fuzz at unaligned windows: the oracle's verdict and bytes, and the guards"""
    _damaged_lz4(gpu, oracle, W.lz4_fuzz_cases(oracle))


def test_lz4_block_parallel_decode_damaged_payloads_stay_in_their_windows(gpu, oracle):
    """the same for test_lz4_block_parallel_decoder_differential_fuzz (payloads of several units, the oracle's and the HIP encoder's)"""
    raws = W.lz4_pd_fuzz_raws(oracle)
    _damaged_lz4(gpu, oracle, W.lz4_pd_fuzz_cases(oracle, raws, encode(gpu.lz4_compress_blocks, raws, W.lz4_bound)))


# ---- zstd decode --------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def zstd_frames(gpu, oracle, ref):
    """{"own": [(frame, raw)] of the product encoder at qualities 0, 1, 2 (+ a chain of eight pieces at quality 2),
    "reference": [(frame, raw)] of the reference encoder at settings 0 and 2}"""
    raws = W.zstd_raws(oracle)
    own = []
    for q in (0, 1, 2):
        rr = raws + ([oracle.synth(W.ZSTD_CHAIN_SIZE, 77, 12)] if q == 2 else [])
        own += list(zip(encode(lambda *a, q=q: gpu.zstd_compress_blocks(*a, quality=q), rr, W.zstd_bound), rr))
    assert all(len(f) > 0 for f, _ in own)
    theirs = [(ref.compress(1, ref.dll.refh_zstd_type(w), r), r) for w in (0, 2) for r in raws]
    return {"own": own, "reference": theirs}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("who", ["own", "reference"])
def test_zstd_decode_valid_frames_stay_in_their_windows(gpu, zstd_frames, mode, who):
    """5 destination residues x 3 source residues, capacity = content size: the raws, the guards; own frames stay on the lane decoders,
    the reference's frames are listed for the block-parallel decoder."""
    cases = [(f, r, s, d) for f, r in zstd_frames[who] for d in W.ZSTD_DEC_DST_RES for s in W.ZSTD_DEC_SRC_RES]
    lay = W.build_layout([f for f, _, _, _ in cases], [(s, d, len(r)) for _, r, s, d in cases], mode)
    check(lay, W.run(lay, gpu.zstd_decompress_blocks), [r for _, r, _, _ in cases])
    n_pay, n_blocks, n_back, where = gpu.zstd_last_decode_stats()
    assert n_pay == len(cases)
    if who == "own":
        assert n_back == 0, (n_back, where)  # none went back to the serial decoder
    else:
        assert n_blocks >= sum((len(r) + 131071) // 131072 for _, r, _, _ in cases)  # (a block holds at most 128 KiB)


@pytest.mark.parametrize("mode", MODES)
def test_zstd_decode_refuses_frames_that_want_more_room(gpu, zstd_frames, mode):
    """capacity = content - {1, 16, 4096, 131072}: refused, and nothing outside the smaller window"""
    blocks, specs = [], []
    for f, r in zstd_frames["own"] + zstd_frames["reference"]:
        for short in W.ZSTD_SHORT_BY:
            if len(r) - short > 0:
                i = len(blocks)
                blocks.append(f), specs.append((W.ZSTD_DEC_SRC_RES[i % 3], 1 + i % 15, len(r) - short))
    lay = W.build_layout(blocks, specs, mode)
    check(lay, W.run(lay, gpu.zstd_decompress_blocks), [None] * len(blocks))


@pytest.fixture
def zstd_model(oracle):
    """ltz_model_decompress in the product's frame layout (sub-blocks, no repeat codes), as the zmode fixture of test_gpu_codecs.py sets it"""
    d = oracle.dll
    d.ltz_model_sub_blocks.argtypes, d.ltz_model_sub_blocks.restype = [C.c_int], None
    d.ltz_model_flags.argtypes, d.ltz_model_flags.restype = [C.c_uint32], None
    d.ltz_model_decompress.restype = C.c_int
    d.ltz_model_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    d.ltz_model_sub_blocks(1)
    d.ltz_model_flags(0)
    yield d
    d.ltz_model_sub_blocks(0)


def test_zstd_decode_damaged_frames_stay_in_their_windows(gpu, oracle, ref, zstd_model):
    """the damaged frames of test_zstd_decoder_agrees_with_host_model_and_reference_on_damaged_frames at unaligned windows: the host
    model's verdict and bytes, and the guards"""
    cases = W.zstd_damaged_frames(oracle, ref)
    expect = []
    for f, cap in cases:
        buf = np.zeros(cap + 8, np.uint8)
        m = C.c_size_t(0)
        e = zstd_model.ltz_model_decompress(f.ctypes.data, len(f), buf.ctypes.data, cap, C.byref(m))
        expect.append(None if e != 0 else buf[: m.value])
    lay = W.build_layout([f for f, _ in cases], [(i % 16, 1 + i % 15, cap) for i, (_, cap) in enumerate(cases)], "guarded")
    check(lay, W.run(lay, gpu.zstd_decompress_blocks), expect)
    assert 20 < sum(e is not None for e in expect) < len(cases)


# ---- LZ4 compress -------------------------------------------------------------------------------------------------------------------


def _lz4_payloads_decode(oracle, lay, results, raws):
    """every payload of a call with room decodes to its source with the oracle (and the reference where it is built)"""
    for res in results:
        for b, raw in enumerate(raws):
            s = int(res.sizes[b])
            assert 0 < s <= lay.caps[b], (s, lay.describe(b))
            p = res.windows[b][:s].copy()
            n, out = oracle.lz4_decompress(p, len(raw))
            assert n == len(raw) and (out == raw).all(), lay.describe(b)
            if have_ref():
                err, out2 = get_ref().decompress(0, p, len(raw))
                assert err == 0 and len(out2) == len(raw) and (out2 == raw).all(), lay.describe(b)


def _same_payloads(lay, results):
    """both calls of a run gave the same payloads -> (sizes, payloads)"""
    a, b = results
    assert (a.sizes == b.sizes).all(), "the encoder's payload sizes differ between two calls with the same input"
    pay = [w[: int(s)].copy() for w, s in zip(a.windows, a.sizes)]
    for i, (p, w) in enumerate(zip(pay, b.windows)):
        assert (w[: len(p)] == p).all(), f"the encoder's payload differs between two calls with the same input, {lay.describe(i)}"
    return a.sizes.astype(np.int64), pay


@pytest.mark.parametrize("mode", MODES)
def test_lz4_compress_stays_in_its_windows_at_every_capacity(gpu, oracle, mode):
    """4 source residues x 16 destination residues x 11 sizes x 3 kinds.  With the bound as capacity the payloads decode to the
    sources (sizes S0); capacity S0 gives the same payload, S0 - 1, S0 / 2 and 0 give 0; no call touches a byte outside a window."""
    cases = W.enc_cases(oracle, W.LZ4_ENC_SIZES, W.LZ4_ENC_KINDS)
    raws = [r for r, _, _, _ in cases]
    full = W.build_layout(raws, [(s, d, W.lz4_bound(len(r))) for r, s, d, _ in cases], mode)
    results = W.run(full, gpu.lz4_compress_blocks)
    W.check_guards(full, results)
    _lz4_payloads_decode(oracle, full, results, raws)
    s0, pay = _same_payloads(full, results)
    for caps, expect in ((s0, pay), (s0 - 1, [0] * len(raws)), (s0 // 2, [0] * len(raws)), (s0 * 0, [0] * len(raws))):
        lay = W.build_layout(raws, [(s, d, int(c)) for (_, s, d, _), c in zip(cases, caps)], mode, same_source=full)
        check(lay, W.run(lay, gpu.lz4_compress_blocks), expect)


@pytest.mark.parametrize("mode", MODES)
def test_lz4_compress_noise_with_capacities_inside_the_speculative_placement(gpu, oracle, mode):
    """A noise block is one literal run, placed 4 KiB unit by unit before the encoder knows that the payload fits: capacities that end at
    the start of, one byte into and one byte before the end of the first, second and sixteenth unit give the payload where it fits and 0
    where it does not, and nothing past the capacity either way."""
    cases = [c for c in W.enc_cases(oracle, W.LZ4_ENC_SIZES, W.LZ4_ENC_KINDS) if c[3] == 0]
    raws = [r for r, _, _, _ in cases]
    full = W.build_layout(raws, [(s, d, W.lz4_bound(len(r))) for r, s, d, _ in cases], mode)
    results = W.run(full, gpu.lz4_compress_blocks)
    W.check_guards(full, results)
    _lz4_payloads_decode(oracle, full, results, raws)
    s0, pay = _same_payloads(full, results)
    for k in range(9):
        caps = [W.lz4_noise_cut_caps(len(r))[k] for r in raws]
        lay = W.build_layout(raws, [(s, d, c) for (_, s, d, _), c in zip(cases, caps)], mode, same_source=full)
        check(lay, W.run(lay, gpu.lz4_compress_blocks), [p if c >= len(p) else 0 for p, c in zip(pay, caps)])


# ---- zstd compress ------------------------------------------------------------------------------------------------------------------

SKIPPABLE = bytes([0x5D, 0x2A, 0x4D, 0x18])  # the magic of the skippable frame that holds the directory (k_zstd.hip)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("quality", [0, 1, 2])
def test_zstd_compress_stays_in_its_windows_at_every_capacity(gpu, oracle, ref, mode, quality):
    """4 source residues x 16 destination residues x 6 sizes x 4 kinds.  With the bound as capacity the frames decode with the reference
    (sizes S0) and end with the directory trailer of T bytes; by k_zstd_scan, capacity >= S0 gives that frame, S0 - T <= capacity < S0
    the frame without the trailer -- a standard frame: the reference and this library decode it --, anything smaller 0."""
    cases = W.enc_cases(oracle, W.ZSTD_ENC_SIZES, W.ZSTD_ENC_KINDS)
    raws = [r for r, _, _, _ in cases]
    call = lambda *a: gpu.zstd_compress_blocks(*a, quality=quality)
    full = W.build_layout(raws, [(s, d, W.zstd_bound(len(r))) for r, s, d, _ in cases], mode)
    results = W.run(full, call)
    W.check_guards(full, results)
    s0, frames = _same_payloads(full, results)
    t = np.array([W.zstd_trailer_size(len(r)) if len(r) else 0 for r in raws], np.int64)  # (an empty block's frame carries none)
    for b, (f, raw) in enumerate(zip(frames, raws)):
        assert 0 < len(f) <= full.caps[b], full.describe(b)
        err, out = ref.decompress(1, f, len(raw))
        assert err == 0 and len(out) == len(raw) and (out == raw).all(), full.describe(b)
        if t[b]:
            tail = bytes(f[len(f) - int(t[b]) :])
            assert tail[:4] == SKIPPABLE and int.from_bytes(tail[4:8], "little") == t[b] - 8 and tail[8:11] == b"LTP", full.describe(b)
    bare = [f[: len(f) - int(k)] for f, k in zip(frames, t)]  # the frames without their trailers
    for b, (f, raw) in enumerate(zip(bare, raws)):
        err, out = ref.decompress(1, f, len(raw))
        assert err == 0 and len(out) == len(raw) and (out == raw).all(), full.describe(b)
    none = [0] * len(raws)
    for caps, expect in ((s0, frames), (s0 - 1, [f if k else 0 for f, k in zip(bare, t)]), (s0 - t, bare), (s0 - t - 1, none),
                         (np.full(len(raws), 13), none), (s0 * 0, none)):
        lay = W.build_layout(raws, [(s, d, int(c)) for (_, s, d, _), c in zip(cases, caps)], mode, same_source=full)
        check(lay, W.run(lay, call), expect)
    # ... and this library's decoder reads the frames without trailers (one per size and kind)
    one = [b for b, (_, s, d, _) in enumerate(cases) if s == 1 and d == 1 and len(raws[b])]
    lay = W.build_layout([bare[b] for b in one], [(1, 1, len(raws[b])) for b in one], mode)
    check(lay, W.run(lay, gpu.zstd_decompress_blocks), [raws[b] for b in one])
