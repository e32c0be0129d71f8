"""-m gpu: the sources of tests/zstd_encoder_sources.py through lthip_zstd_compress_blocks.

Quality 0, the whole table in one call on the guarded layouts of tests/codec_windows_util.py (sources at every residue mod 16,
destination windows of zstd_bound at odd offsets between guard bytes, two fills): every frame has a size within the bound, is the same
on both fills, decodes to its source with the reference and with zstd_decompress_blocks, and every Compressed piece is, byte for byte,
what the host model (oracle/zstd_model.c, the same zstd_block_core.h with one lane) makes of the GPU match finder's OWN units
(zstd_debug_units).  Coverage is counted from the GPU's frames (tests/zstd_format.py: census), per family: the keys the family's cases
claim occur.  A key of family (b) the match finder cannot be brought to produce stands in MATCH_FINDER_EXEMPT with the reason seen in
zstd_debug_units; a key of that list that does turn up fails the test, so the list cannot go stale.  Families (a), (c) and (d) have no
such list: where the executed bytes of a unit case miss a corner, tests/zstd_encoder_sources.py places a source by the match finder's
rules.  (The directory version is 4 at quality 2 only, LTHIP_ZSTD_Q_MAX in k_zstd.hip; qualities 0 and 1 write version 2.)

Multi-piece frames (k_zstd_scan, k_zstd_emit, the directory) at qualities 0, 1 and 2: the directory entries are the block sizes, pieces
of one Raw_Block / RLE_Block say so, Last_Block is on the last block only, and a block's frame is the same alone, in a list, in the
reversed list and in the doubled list."""
from collections import Counter

import numpy as np
import pytest

from tests import codec_windows_util as W
from tests import zstd_encoder_sources as S
from tests import zstd_format as Z
from tests.zstd_gpu_util import check_against_model, model_compress, model_src, zstd_pieces

pytestmark = pytest.mark.gpu

# census keys of family (b) that the GPU's frames of the table do not hold, with what zstd_debug_units shows instead
_COUNTS = ("the parser takes its own candidates (aligned dwords enter its tables): of the 127 .. 1024 short matches at random distances put "
           "into the unit it finds 37 .. 126, with longer literal runs between")
_LONG = ("a match of 39 .. 1026 bytes at distance 50 is found as the period it is: one sequence of the unit's rest (unit meta: 1 sequence "
         "where 58 were put), so these lengths' codes do not occur")
_FAR = "of the 30 offsets put into the unit 5 are found, none further back than 16 380 (a lone far repeat is not looked at)"
_MANY = "accuracy log 9 needs 1024 sequences in a piece: of the 1106 put in, the parser finds 575"
MATCH_FINDER_EXEMPT = {
    **{f"nbseq_{n}": _COUNTS for n in (127, 128, 255, 256, 1023, 1024)},
    **{f"ml_code_{c}": _LONG for c in (36, 37, 38, 40, 41, 42, 43, 45)},
    **{f"of_code_{c}": _FAR for c in (14, 15, 16)},
    "ll_fse_log_9": _MANY, "ml_fse_log_9": _MANY,
    "lit_n0": "the unit that is one match of 4096 bytes from 65 535 back: the parser leaves its half-group without a sequence",
}

def encode(gpu, datas, quality=0, residues=None):
    """one call on a guarded layout, twice (two fills) -> the frames; asserts the guards, the sizes and that both runs agree"""
    res = residues if residues is not None else [i % 16 for i in range(len(datas))]
    lay = W.build_layout(list(datas), [(res[i], (2 * i + 1) % 16, W.zstd_bound(len(d))) for i, d in enumerate(datas)], "guarded")
    assert all(o % 2 for o in lay.dst_offs)
    first, second = W.run(lay, lambda *a: gpu.zstd_compress_blocks(*a, quality=quality))
    W.check_guards(lay, (first, second))
    out = []
    for b in range(len(datas)):
        s = int(first.sizes[b])
        assert 0 < s <= lay.caps[b], f"size {s}, {lay.describe(b)}"
        assert s == int(second.sizes[b]) and (first.windows[b][:s] == second.windows[b][:s]).all(), f"{lay.describe(b)}: the frame depends on what the window held"
        out.append(first.windows[b][:s].copy())
    return out


def decode_both(gpu, ref, datas, frames, way):
    bad = []
    for i, (d, f) in enumerate(zip(datas, frames)):
        err, out = ref.decompress(1, f, len(d))
        if err != 0 or len(out) != len(d) or not (out == d).all():
            bad.append(f"source {i}: the reference decodes with error {err}, {len(out)} bytes")
    lay = W.build_layout(frames, [(i % 16, (2 * i + 1) % 16, len(d)) for i, d in enumerate(datas)], "guarded")
    results = W.run(lay, gpu.zstd_decompress_blocks)
    W.check_guards(lay, results)
    for res in results:
        for b, d in enumerate(datas):
            if int(res.sizes[b]) != len(d) or not (res.windows[b][: len(d)] == d).all():
                bad.append(f"source {b}: zstd_decompress_blocks gives {int(res.sizes[b])} bytes")
    assert not bad, f"{way}: {len(bad)} frames do not decode to their sources, the first: " + "; ".join(bad[:10])


@pytest.fixture(scope="module")
def table(gpu, oracle):
    """the table's frames at quality 0, and how many Compressed pieces equal the host model: the model is run here, straight after
    the call whose units zstd_debug_units still holds"""
    datas = [s.data for s in S.sources()]
    frames = encode(gpu, datas)
    d = model_src(oracle)
    oracle.dll.ltz_model_sub_blocks(1)
    try:
        checked = check_against_model(gpu, d, datas, frames)
    finally:
        oracle.dll.ltz_model_sub_blocks(0)
    return frames, checked


def test_table_at_quality_0(gpu, ref, table):
    srcs = S.sources()
    frames, checked = table
    assert checked >= len([s for s in srcs if not s.zero]) * 3 // 4, "too few Compressed pieces were compared with the host model"
    decode_both(gpu, ref, [s.data for s in srcs], frames, "the table at quality 0")


def test_coverage_per_family_from_the_gpus_frames(table):
    srcs = S.sources()
    frames = table[0]
    found = {fam: Counter() for fam in S.FAMILIES}
    for s, f in zip(srcs, frames):
        found[s.family] += Z.census(bytes(f))
    missing = {}
    for fam in S.FAMILIES:
        want = sorted({k for s in srcs if s.family == fam for k in s.has})
        print(f"zstd encoder sources, family ({fam}): {len(want)} claimed keys, the GPU's frames hold {sum(1 for k in want if found[fam][k])}")
        lack = [k for k in want if not found[fam][k] and not (fam == "b" and k in MATCH_FINDER_EXEMPT)]  # (no exemption but (b)'s)
        if lack:
            missing[fam] = lack
    print(f"zstd encoder sources: keys the GPU's frames do not hold: {missing}")
    stale = [k for k in MATCH_FINDER_EXEMPT if found["b"][k]]
    assert not stale, f"listed as not reached, and found: {stale}"
    assert not missing, f"keys the GPU's frames do not hold: {missing}"
    d = [f"{s}_stream_{w}" for s in ("lit", "seq") for w in [f"start_mod4_{r}" for r in range(4)] + [f"endbit_mod32_{b}" for b in range(32)]]
    assert not [k for k in d if not found["d"][k]], [k for k in d if not found["d"][k]]


def test_sizes_per_family(oracle, table):
    """on record, not asserted: GPU frame bytes beside the host model's with its greedy matcher"""
    srcs = S.sources()
    frames = table[0]
    oracle.dll.ltz_model_sub_blocks(1)
    try:
        for fam in S.FAMILIES:
            g = sum(len(f) for s, f in zip(srcs, frames) if s.family == fam)
            m = sum(len(model_compress(oracle, s.data)) for s in srcs if s.family == fam)
            print(f"zstd encoder sources, family ({fam}): GPU {g} bytes of frames, host model {m}, sources {sum(len(s.data) for s in srcs if s.family == fam)}")
    finally:
        oracle.dll.ltz_model_sub_blocks(0)


# ---- frames of several pieces ------------------------------------------------------------------------------------------------------------
def directory(frame):
    """(version, u16 entries) of the frame's directory trailer, or (0, None)"""
    content = int.from_bytes(bytes(frame[5:13]), "little")
    nunits = (content + 4095) // 4096
    tail = bytes(frame[len(frame) - 12 - 2 * nunits :])
    if nunits and tail[:4] == bytes([0x5D, 0x2A, 0x4D, 0x18]) and tail[8:11] == b"LTP":
        return tail[11], np.frombuffer(tail[12:], dtype="<u2")
    return 0, None


@pytest.mark.parametrize("quality", [0, 1, 2])
def test_frames_of_several_pieces(gpu, oracle, ref, quality):
    table = S.frames()
    datas = [d for _, d, _ in table]
    res = [(5 * i + 3) % 16 for i in range(len(datas))]
    frames = encode(gpu, datas, quality, res)
    decode_both(gpu, ref, datas, frames, f"frames of several pieces, quality {quality}")
    for (name, d, kinds), f in zip(table, frames):
        c = Z.census(bytes(f))
        assert c["last_raw"] + c["last_rle"] + c["last_compressed"] == 1 and c["skippable_last"] == 1, name
        ver, entries = directory(f)
        assert ver == (4 if quality == 2 else 2), f"'{name}': directory version {ver}"
        pieces = zstd_pieces(f, versions=(4 if quality == 2 else 2,))  # (walks the blocks and holds every directory entry against its block's header)
        assert len(pieces) == (len(d) + S.PIECE - 1) // S.PIECE, name
        if kinds:
            for i, k in enumerate(kinds):
                e = entries[32 * i : 32 * i + 32]
                want = S.KIND_DIRECTORY[k]
                if want is None:
                    assert (e < 0xFFFE).all() and pieces[i][0] == 2, f"'{name}': piece {i} is no run of sub-blocks"
                else:
                    assert (e == want).all() and pieces[i][0] == (1 if k == "rle" else 0), f"'{name}': piece {i} ({k}) has entries {sorted(set(e.tolist()))[:4]}"
    # one block's frame does not depend on its company or its place
    pick = [0, 5, 7, 10, 16, len(datas) - 5, len(datas) - 3, len(datas) - 1]
    for order, idx in (("alone", [[i] for i in pick]), ("list", [pick]), ("reversed", [pick[::-1]]), ("doubled", [pick + pick])):
        for group in idx:
            got = encode(gpu, [datas[i] for i in group], quality, [res[i] for i in group])
            for k, i in enumerate(group):
                assert len(got[k]) == len(frames[i]) and (got[k] == frames[i]).all(), f"quality {quality}, {order}: the frame of '{table[i][0]}' differs"
