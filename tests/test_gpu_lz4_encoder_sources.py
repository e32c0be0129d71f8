"""-m gpu: the hand-built sources of tests/lz4_encoder_sources.py (every corner of the block format's field boundaries, of the end-of-block
rules and of the parser's units, groups and scan steps) through lthip_lz4_compress_blocks:
  (a) the product library at the default unit (classification pass, lane parser, stitch);
  (b) the product library with segment_log2 10, 11 and 13: the batch parser for everything.
Sources lie at every residue mod 16, destination windows of lz4_bound at odd offsets between guard bytes (tests/codec_windows_util.py),
on two fills.  Every payload has a size within the bound, is the same on both fills, decodes to its source with the oracle (and the
reference where it is built) and keeps the rules an ENCODER owes and no decoder checks (Z.encoder_rules: the last match starts 12 bytes
and ends 5 bytes before the end, offsets within 1 .. 65535, one coding per length).  The union of the payloads' fields of (a) holds
every boundary the table is built for (S.Coverage; tests/test_lz4_encoder_sources_cases.py holds the oracle's payloads to the same).
Further: a block's payload does not depend on the order of the call's blocks or on its company (k_lz4.hip: "results do not depend on
timing"); the same sources through zstd_compress_blocks at qualities 0, 1, 2 decode with the reference and with this library; sources
of a period of 8 and less compress to under a quarter; the ablation library, with no switch set, writes the product's bytes."""
import numpy as np
import pytest

from tests import codec_windows_util as W
from tests import lz4_encoder_sources as S
from tests import lz4_format as Z
from tests._libs import have_ref, ref as get_ref

pytestmark = pytest.mark.gpu


def encode(call, datas, bound, residues=None):
    """one call on a guarded layout, twice (two fills) -> the payloads; asserts the guards, the sizes and that both runs agree"""
    res = residues if residues is not None else [i % 16 for i in range(len(datas))]
    lay = W.build_layout(list(datas), [(res[i], (2 * i + 1) % 16, bound(len(d))) for i, d in enumerate(datas)], "guarded")
    assert all(o % 2 for o in lay.dst_offs) and (residues is not None or {o % 16 for o in lay.src_offs} == set(range(min(16, len(datas)))))
    first, second = W.run(lay, call)
    W.check_guards(lay, (first, second))
    out = []
    for b in range(len(datas)):
        s = int(first.sizes[b])
        assert 0 < s <= lay.caps[b], f"size {s}, {lay.describe(b)}"
        assert s == int(second.sizes[b]), f"sizes {s} and {int(second.sizes[b])} on two fills, {lay.describe(b)}"
        assert (first.windows[b][:s] == second.windows[b][:s]).all(), f"{lay.describe(b)}: the payload depends on what the window held"
        out.append(first.windows[b][:s].copy())
    return out


def check_payloads(oracle, srcs, payloads, way):
    """every payload decodes to its source and keeps the encoder's rules; all the failures of a run in one report"""
    r = get_ref() if have_ref() else None
    bad = []
    for s, p in zip(srcs, payloads):
        n, out = oracle.lz4_decompress(p, len(s.data))
        if n != len(s.data) or not (out == s.data).all():
            bad.append(f"'{s.name}': the oracle decodes {n} bytes" + ("" if n != len(s.data) else ", other than the source's"))
            continue
        if r is not None:
            err, out2 = r.decompress(0, p, len(s.data))
            if err != 0 or len(out2) != len(s.data) or not (out2 == s.data).all():
                bad.append(f"'{s.name}': the reference decodes with error {err}, {len(out2)} bytes")
        fields, broken = Z.encoder_rules(p.tobytes(), len(s.data))
        if broken:
            bad.append(f"'{s.name}' ({len(s.data)} bytes): {broken[:3]}")
    assert not bad, f"{way}: {len(bad)} of {len(srcs)} payloads, the first: " + "; ".join(bad[:12])


def ratios(oracle, srcs, payloads, way):
    """the floor: a source of a period of 8 and less, one unit and longer, compresses to under a quarter (test_lz4_structured_inputs
    holds 65 539 zeros to under 2000 bytes, eight times tighter); per family, GPU size / oracle size on record in the log"""
    fat = [f"'{s.name}': {len(p)} of {len(s.data)}" for s, p in zip(srcs, payloads) if s.short_period and 4 * len(p) >= len(s.data)]
    for fam in S.FAMILIES:
        g = sum(len(p) for s, p in zip(srcs, payloads) if s.family == fam)
        o = sum(len(oracle.lz4_compress(s.data)) for s in srcs if s.family == fam)
        print(f"lz4 encoder sources, {way}, family '{fam}': GPU {g} / oracle {o} = {g / o:.3f}")
    assert not fat, f"{way}: {len(fat)} sources of a short period stay above a quarter, the first: " + "; ".join(fat[:8])


_product = {}


def product_payloads(gpu):
    if "p" not in _product:
        _product["p"] = encode(gpu.lz4_compress_blocks, [s.data for s in S.sources()], W.lz4_bound)
    return _product["p"]


def product_frames(gpu, quality):
    if ("z", quality) not in _product:
        _product["z", quality] = encode(lambda *a: gpu.zstd_compress_blocks(*a, quality=quality), [s.data for s in S.sources()], W.zstd_bound)
    return _product["z", quality]


def test_product_library_default_unit(gpu, oracle):
    """(a); run before the tests below, which read its payloads"""
    srcs = S.sources()
    check_payloads(oracle, srcs, product_payloads(gpu), "product, default unit")


def test_coverage_of_the_product_payloads(gpu):
    """the field boundaries are in the GPU's payloads, not only in the oracle's; no offset field is 0 (the period-G source, the repeat
    exactly G back: a distance the field cannot hold must not wrap)"""
    srcs = S.sources()
    cov = S.Coverage()
    for s, p in zip(srcs, product_payloads(gpu)):
        cov.add(s, Z.loose(p.tobytes())[0])
    print(f"lz4 encoder sources, product: literal lengths {sorted(v for v in cov.lit_lens if v < 600)[:80]}, match lengths "
          f"{sorted(v for v in cov.match_lens if v < 600)[:80]}, offsets below 10 {sorted(v for v in cov.offsets if v < 10)}, the largest "
          f"{max(cov.offsets)}, the longest literal run {max(cov.lit_lens)}, ends at n - 5: {len(cov.ends_at_5)}, starts at n - 12: {len(cov.starts_at_12)}")
    assert cov.missing() == [], cov.missing()
    for name in (f"period {S.G} over two periods + 5000 bytes", f"the only repeat lies {S.G} back"):
        p = product_payloads(gpu)[[s.name for s in srcs].index(name)]
        assert all(e["off"] is None or 1 <= e["off"] < S.G for e in Z.loose(p.tobytes())[0]), name


def test_ratio_floor_and_the_families_ratios(gpu, oracle):
    ratios(oracle, S.sources(), product_payloads(gpu), "product, default unit")


@pytest.mark.parametrize("log2", [10, 11, 13])
def test_other_unit_sizes(gpu, oracle, log2):
    """(b) segment_log2 other than 12 keeps the batch parser's geometry for every group: the same checks"""
    srcs = S.sources()
    pay = encode(lambda *a: gpu.lz4_compress_blocks(*a, segment_log2=log2), [s.data for s in srcs], W.lz4_bound)
    check_payloads(oracle, srcs, pay, f"segment_log2 = {log2}")
    ratios(oracle, srcs, pay, f"segment_log2 = {log2}")


def test_order_and_company(gpu, oracle):
    """Each batch list (an empty block, blocks of 1, 12 and 13 bytes, a block without a match -- laid out by the match finder, never
    seen by the copy kernel --, a matched block, the 70-unit block), its reverse and its doubled form: a block's payload is the same in
    every list and the same as alone.  (A block keeps its source residue throughout: the parse may depend on the source's alignment.)"""
    blocks = S.batch_blocks()
    res = [(3 * i + 1) % 16 for i in range(len(blocks))]
    alone = [encode(gpu.lz4_compress_blocks, [d], W.lz4_bound, [res[i]])[0] for i, (_, d) in enumerate(blocks)]
    for (name, d), p in zip(blocks, alone):
        n, out = oracle.lz4_decompress(p, len(d))
        assert n == len(d) and (out == d).all() and Z.encoder_rules(p.tobytes(), len(d))[1] == [], name
    assert len(alone[0]) == 1 and alone[0][0] == 0 and len(alone[4]) == W.lz4_literal_run_size(len(blocks[4][1]))  # (empty; no match)
    for i in (5, 6):  # (the matched routes: the copy kernel places them)
        assert any(e["off"] is not None for e in Z.loose(alone[i].tobytes())[0]), blocks[i][0]
    for which, idx in S.batches().items():
        got = encode(gpu.lz4_compress_blocks, [blocks[i][1] for i in idx], W.lz4_bound, [res[i] for i in idx])
        for k, i in enumerate(idx):
            assert len(got[k]) == len(alone[i]) and (got[k] == alone[i]).all(), (
                f"list '{which}', place {k}: the payload of '{blocks[i][0]}' ({len(got[k])} bytes) is not the one it has alone ({len(alone[i])} bytes)")


@pytest.mark.parametrize("quality", [0, 1, 2])
def test_zstd_front_end(gpu, ref, quality):
    """the same sources through the match finder's zstd flavour (qualities 1 and 2: the history halves reach a group further back, where
    the periods of 2 G and the repeat exactly G back lie): the frames decode with the reference and with this library"""
    srcs = S.sources()
    frames = product_frames(gpu, quality)
    bad = []
    for s, f in zip(srcs, frames):
        err, out = ref.decompress(1, f, len(s.data))
        if err != 0 or len(out) != len(s.data) or not (out == s.data).all():
            bad.append(f"'{s.name}': error {err}, {len(out)} bytes")
    assert not bad, f"quality {quality}: the reference does not decode {len(bad)} frames to their sources, the first: " + "; ".join(bad[:12])
    lay = W.build_layout(frames, [(i % 16, (2 * i + 1) % 16, len(s.data)) for i, s in enumerate(srcs)], "guarded")
    results = W.run(lay, gpu.zstd_decompress_blocks)
    W.check_guards(lay, results)
    for res in results:
        for b, s in enumerate(srcs):
            if int(res.sizes[b]) != len(s.data) or not (res.windows[b] == s.data).all():
                bad.append(f"'{s.name}': {int(res.sizes[b])} bytes")
    assert not bad, f"quality {quality}: zstd_decompress_blocks does not decode {len(bad)} frames to their sources, the first: " + "; ".join(bad[:12])
    g = sum(len(f) for f in frames)
    print(f"lz4 encoder sources, zstd quality {quality}: {g} bytes of frames for {sum(len(s.data) for s in srcs)}")


def test_ablation_library_without_a_switch_writes_the_products_bytes(gpu, gpu_abl):
    """The premise of every gpu_abl differential test: with no LTHIP_* switch set the ablation build runs the product's match finder --
    the same kernels launched the same way, its switches at their defaults.  Every LZ4 payload at the default unit and every zstd frame
    at qualities 0, 1 and 2 is byte for byte the product library's."""
    gpu_abl.lib.dll.lthip_debug_reload_env()  # (a value an earlier test's switch left cached in that library)
    srcs = S.sources()
    datas = [s.data for s in srcs]
    runs = [("lz4", product_payloads(gpu), encode(gpu_abl.lz4_compress_blocks, datas, W.lz4_bound))]
    for q in (0, 1, 2):
        runs.append((f"zstd quality {q}", product_frames(gpu, q), encode(lambda *a: gpu_abl.zstd_compress_blocks(*a, quality=q), datas, W.zstd_bound)))
    bad = []
    for way, prod, abl in runs:
        assert len(prod) == len(abl) == len(srcs)
        bad += [f"{way}, '{s.name}': {len(a)} bytes against the product's {len(p)}" for s, p, a in zip(srcs, prod, abl) if len(p) != len(a) or not (p == a).all()]
    assert not bad, f"{len(bad)} outputs of the ablation library are not the product's, the first: " + "; ".join(bad[:12])
