"""-m gpu: the hand-built zstd frames of tests/zstd_format_frames.py (every format corner, and the near misses one step outside) through
lthip_zstd_decompress_blocks, every way the library has of decoding them:
  (a) the product library as called: few blocks, so the scalar-unit walker (k_zstd_blk_seq_scalar);
  (b) the product library with the case list replicated into one call, so that the call's block count passes the two thresholds of
      k_zstd_decode.hip (`n <= 2 * CUs`: scalar unit; `n <= 4 * nwg`: zs_seq_lanes<0> inline in k_zstd_blk_entropy; above:
      k_zstd_blk_sequences, 64 blocks per wave) -- the product build has no switch for them;
  (c) - (f) the ablation build with LTHIP_ZSTD_SEQ_SCALAR=2 / =0, LTHIP_ZSTD_DBG=16 (a payload's blocks in order on one wave
      instead of origins) and LTHIP_ZSTD_DBG=1 (serial).
What is expected comes from the CPU side alone (tests/test_zstd_format_cases.py proves it against the reference): a valid frame gives
its content size and the bytes the writer computed, a near miss is refused -- the host model's verdict --, the wrong content checksum
is skipped.  Payloads lie at every source residue mod 16 (the first at 0), destination windows at odd offsets between guard bytes
(tests/codec_windows_util.py): nothing outside the windows is written, whatever the verdict."""
import numpy as np
import pytest
import torch

from tests import codec_windows_util as W
from tests import zstd_format as Z
from tests import zstd_format_frames as F

pytestmark = pytest.mark.gpu
ZB = 131072


def entry(name, cap_delta=0, refused=False):
    """(case, destination capacity, expected bytes | None = refused)"""
    c = next(c for c in F.CASES if c["name"] == name)
    _, out = F.built(name)
    ok = c["verdict"] in ("valid", "checksum") and not refused
    return c, F.capacity(c) + cap_delta, (out if ok else None)


SMALL = [entry(c["name"]) for c in F.CASES if not c["large"]]
LARGE = [entry(c["name"]) for c in F.CASES if c["large"]]
# destinations larger than the content (block-parallel, unlisted and handed-back frames), and one byte short: refused
ROOMY = [entry("fcs 4 bytes", 7), entry("every table fse", 1000), entry("two frames", 3), entry(F.DENSE, 70000), entry(F.EIGHT, 1)]
SHORT = [entry(n, -1, refused=True) for n in ("fcs 4 bytes", "repeat after fse", "rle block of 131072", F.DENSE, "two frames", F.EIGHT)]


def decode(ctx, entries):
    """one call on a guarded layout, twice (two fills) -> per entry the bytes or None; asserts the guards and that both runs agree"""
    frames = [np.frombuffer(F.built(c["name"])[0], np.uint8) for c, _, _ in entries]
    specs = [(i % 16, (2 * i + 1) % 16, cap) for i, (_, cap, _) in enumerate(entries)]  # source residues 0, 1, .. 15, 0, ..; odd destinations
    lay = W.build_layout(frames, specs, "guarded")
    assert lay.src_offs[0] == 0 and {o % 16 for o in lay.src_offs} == set(range(min(16, len(entries)))) and all(o % 2 for o in lay.dst_offs)
    first, second = W.run(lay, ctx.zstd_decompress_blocks)
    W.check_guards(lay, (first, second))
    out = []
    for b in range(len(entries)):
        s = int(first.sizes[b])
        assert s == int(second.sizes[b]), lay.describe(b)
        if s == W.REFUSED:
            out.append(None)
        else:
            assert s <= lay.caps[b] and (first.windows[b][:s] == second.windows[b][:s]).all(), lay.describe(b)
            out.append(first.windows[b][:s].tobytes())
    return out


def check(entries, got, way):
    for (c, cap, want), g in zip(entries, got):
        what = f"{way}: '{c['name']}' ({c['verdict']}, capacity {cap})"
        if want is None:
            assert g is None, f"{what} was accepted ({len(g)} bytes)"
        else:
            assert g is not None, f"{what} was refused"
            assert len(g) == len(want), f"{what}: {len(g)} bytes for {len(want)}"
            assert g == want, f"{what}: bytes differ first at {next(i for i in range(len(g)) if g[i] != want[i])}"


def listed_blocks(entries):
    """blocks k_zstd_split lists for the block-parallel path: every block of a valid frame that stays there or is handed back later"""
    return sum(sum(v for k, v in Z.census(F.built(c["name"])[0]).items() if k in ("block_raw", "block_rle", "block_compressed"))
               for c, _, want in entries if want is not None and c["path"] in ("parallel", "handed_back"))


def test_product_library_as_called(gpu):
    """(a), with the destinations larger than the content and one byte short in the same call"""
    entries = SMALL + ROOMY + SHORT
    check(entries, decode(gpu, entries), "product")
    n_pay, n_blocks, _, _ = gpu.zstd_last_decode_stats()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_pay == len(entries) and 0 < n_blocks <= 2 * ncu  # the scalar-unit walker's range (k_zstd_decode.hip: scalar_seqs)
    check(LARGE, decode(gpu, LARGE), "product, large")


def test_what_stays_parallel_and_what_is_declined(gpu):
    """lthip_zstd_last_decode_stats after the product call: [1] the blocks k_zstd_split listed for the block-parallel path, [2] the
    payloads that path handed back to k_zstd_decode_retry (d_retry).  From the code, a valid frame leaves the block-parallel path in
    two ways: z_split_foreign never lists it (no content size, zero content, a second or a skippable frame in the payload, more than
    ZF_SLOTS blocks per 128 KiB of capacity: z_split_walk, the serial decoder, from the start; neither [1] nor [2] counts it), or it is
    listed and handed back (an Offset_Value of 2^24 and more, a record arena that one sequence per three bytes overflows, a literal
    stream without symbols: four streams of six literals).  Either way the serial decoder gives the bytes."""
    valid = [e for e in SMALL + LARGE if e[0]["verdict"] == "valid"]
    parallel = [e for e in valid if e[0]["path"] == "parallel"]
    unlisted = [e for e in valid if e[0]["path"] == "unlisted"]
    handed = [e for e in valid if e[0]["path"] == "handed_back"]
    assert len(parallel) > 40 and len(unlisted) == 7 and [e[0]["name"] for e in handed] == [F.SIX, F.DENSE, "offset value of 2^24 and more"]
    check(parallel, decode(gpu, parallel), "parallel frames")
    n_pay, n_blocks, n_back, where = gpu.zstd_last_decode_stats()
    assert (n_pay, n_blocks, n_back) == (len(parallel), listed_blocks(parallel), 0), where
    # (the frame of 16 MiB in a call of its own: its bytes would size a record arena that holds the dense frame's records)
    for group in (handed[:2], handed[2:]):
        check(group, decode(gpu, group), "handed back")
        n_pay, n_blocks, n_back, where = gpu.zstd_last_decode_stats()
        assert (n_pay, n_blocks, n_back) == (len(group), listed_blocks(group), len(group)), where
    check(unlisted, decode(gpu, unlisted), "never listed")
    n_pay, n_blocks, n_back, where = gpu.zstd_last_decode_stats()
    assert (n_pay, n_blocks, n_back) == (len(unlisted), 0, 0), where
    # every declined frame alone in its call
    for e in unlisted + handed[:2]:
        check([e], decode(gpu, [e]), "alone")
        assert gpu.zstd_last_decode_stats()[1:3] == ((0, 0) if e[0]["path"] == "unlisted" else (1, 1)), e[0]["name"]
    # a declined frame between two parallel ones: all three right, one handed back
    for mid in (entry(F.DENSE), entry("two frames")):
        three = [entry("fcs 4 bytes"), mid, entry("repeat after fse")]
        check(three, decode(gpu, three), "mixed")
        assert gpu.zstd_last_decode_stats()[2] == (1 if mid[0]["path"] == "handed_back" else 0), mid[0]["name"]
    # the record arena is sized from all listed bytes of the call (one record per 6, k_zstd_decode.hip: rec_cap): with two frames of
    # 65791 raw bytes beside it the dense frame's 22000 records fit, and it stays on the block-parallel path
    roomy = [entry(F.DENSE_COMPANION), entry(F.DENSE), entry(F.DENSE_COMPANION)]
    recs = sum(len(e[2]) for e in roomy) // 6 + 64 * listed_blocks(roomy) + 4096
    assert len(F.built(F.DENSE)[1]) // 6 + 64 + 4096 < 22000 <= recs - 64
    check(roomy, decode(gpu, roomy), "dense frame with company")
    assert gpu.zstd_last_decode_stats()[1:3] == (3, 0)


def _replicated(gpu, entries, way):
    check(entries, decode(gpu, entries), way)
    n_pay, n_blocks, _, _ = gpu.zstd_last_decode_stats()
    assert n_pay == len(entries)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    nitems = sum(max(1, (cap + ZB - 1) // ZB) for _, cap, _ in entries)
    return n_blocks, ncu, min(nitems, 8 * ncu)  # (k_zstd_decode.hip: nwg)


def test_product_library_inline_walker(gpu):
    """(b) more than 2 * CUs blocks in the call, at most 4 * nwg: k_zstd_blk_entropy walks the sequences itself (zs_seq_lanes<0>)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    reps = 2 * ncu // listed_blocks(SMALL) + 2
    n_blocks, ncu, nwg = _replicated(gpu, SMALL * reps, "product, inline walker")
    assert 2 * ncu < n_blocks <= 4 * nwg, (n_blocks, ncu, nwg)


def test_product_library_wave_walker(gpu):
    """(b) more than 4 * nwg blocks in the call: k_zstd_blk_sequences, 64 blocks per wave.  nwg is the call's 128 KiB slots (up to
    8 per CU), so the call needs more than four listed blocks per slot: the case list once and many frames of eight blocks."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    entries = SMALL + [entry(F.EIGHT)] * max(120, ncu // 2)
    n_blocks, ncu, nwg = _replicated(gpu, entries, "product, wave walker")
    assert n_blocks > 4 * nwg and n_blocks > 2 * ncu, (n_blocks, ncu, nwg)


@pytest.mark.parametrize("name,value", [("LTHIP_ZSTD_SEQ_SCALAR", "2"), ("LTHIP_ZSTD_SEQ_SCALAR", "0"), ("LTHIP_ZSTD_DBG", "16"), ("LTHIP_ZSTD_DBG", "1")],
                         ids=["scalar-unit walker", "lane walkers", "payload executor", "serial"])
def test_ablation_build_ways(gpu_abl, monkeypatch, name, value):
    """(c) - (f): the same verdicts and bytes"""
    monkeypatch.setenv(name, value)
    gpu_abl.lib.dll.lthip_debug_reload_env()  # (the library caches its switches)
    entries = SMALL + ROOMY + SHORT
    check(entries, decode(gpu_abl, entries), f"{name}={value}")
    check(LARGE, decode(gpu_abl, LARGE), f"{name}={value}, large")
    monkeypatch.delenv(name)
    gpu_abl.lib.dll.lthip_debug_reload_env()
