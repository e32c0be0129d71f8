"""The hand-built zstd frames of tests/zstd_format_frames.py, proved on the CPU to be what they claim before tests/test_gpu_zstd_format.py
sends them through the GPU decoders:
  - the census (tests/zstd_format.py, written from RFC 8878) finds in every valid frame the features it was built for;
  - the REFERENCE decoder (live where oracle/_ref is built, else its recorded answers, tests/golden/ref_results.json) decodes every
    valid frame to the bytes the writer computed by executing its own sequences -- that licenses the writer -- and rejects every near
    miss; the host model of this library's decoder (zstd_decode_core.h, serial) agrees, and is never laxer than the reference but for
    the documented content checksum;
  - the census of the reference encoder's frames for the inputs of tests/test_zstd_model.py::test_decoder_reads_reference_encoder_output
    says which features those fixtures contain (tests/golden/zstd_ref_census.json holds the summary);
  - crafted and reference frames together leave no row of the feature list without a frame."""
import ctypes as C
import json
import os
from collections import Counter

import numpy as np
import pytest

from tests import zstd_format as Z
from tests import zstd_format_frames as F
from tests._libs import GOLDEN, digest, have_ref, ref as get_ref

CENSUS_FILE = GOLDEN / "zstd_ref_census.json"
SEQ_LIMIT = 2000  # sequences decoded per reference frame (every header of every block is read regardless)
IDS = [c["name"] for c in F.CASES]


def model_decode(o, frame: np.ndarray, cap: int):
    o.dll.ltz_model_decompress.restype = C.c_int
    o.dll.ltz_model_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    out = np.zeros(cap + 8, np.uint8)
    n = C.c_size_t(0)
    err = o.dll.ltz_model_decompress(frame.ctypes.data, len(frame), out.ctypes.data, cap, C.byref(n))
    return err, out[: n.value]


def test_toolkit_pieces():
    """XXH64 against its published vectors (inputs of 32 bytes and more: the reference verifies the checksum of the crafted frame);
    table descriptions written and read back; the predefined tables fill their logs."""
    assert Z.xxh64(b"") == 0xEF46DB3751D8E999 and Z.xxh64(b"a") == 0xD24EC4F1A98C6E5B and Z.xxh64(b"abc") == 0x44BC2CF5AD770999
    for t in (Z.LL, Z.OF, Z.ML):
        norm, log = Z.DEFAULTS[t]
        assert sum(abs(c) for c in norm) == 1 << log and len(norm) <= Z.MAX_SYM[t] + 1
        assert Z.default_table(t).symbols() == set(range(len(norm)))
    assert Z.LL_BASE[16:] == [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
    assert Z.ML_BASE[32:] == [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
    rng = np.random.default_rng(5)
    for it in range(300):
        log = int(rng.integers(5, 10))
        nsym = int(rng.integers(2, min(40, (1 << log) + 1)))
        hist = {int(s): int(rng.integers(1, 1000)) for s in rng.choice(53, nsym, replace=False)}
        norm = Z.normalise(hist, log)
        if it % 3 == 0:  # some "less than one" counts
            for s in [s for s, c in enumerate(norm) if c == 1][:3]:
                norm[s] = -1
        d = Z.write_ncount(norm, log)
        back, log2, used = Z.read_ncount(d + b"\xAA", 52, 9)
        assert (back, log2, used) == (norm, log, len(d)), (norm, log)
        tab = Z.FseTable(norm, log)
        for s in tab.symbols():  # every next state has exactly one predecessor state per symbol
            assert all(tab.state_for(s, k) is not None for k in range(1 << log))


@pytest.mark.parametrize("case", F.CASES, ids=IDS)
def test_crafted_frame(case, oracle, refcall):
    data, expected = F.built(case["name"])
    frame = np.frombuffer(data, np.uint8).copy()
    cap = F.capacity(case)

    def decode(r):
        err, out = r.decompress(1, frame, cap)
        return [int(err), len(out), digest(out)]

    ref_answer = refcall("zstd_decompress", [frame, cap], decode)
    want = None if expected is None else [0, len(expected), digest(np.frombuffer(expected, np.uint8))]
    err, out = model_decode(oracle, frame, cap)
    model_answer = [0, len(out), digest(out)] if err == 0 else None
    verdict = case["verdict"]
    if verdict == "valid":
        found = Z.census(data)
        missing = [k for k in case["features"] if not found[k]]
        assert not missing, f"the census does not find {missing} in the frame built for them"
        assert want is not None, "the writer could not execute its own sequences"
        assert ref_answer == want, "the reference does not decode the crafted frame to the writer's bytes: a writer bug"
        assert model_answer == want
        e2, o2 = model_decode(oracle, frame, cap + 5)  # a larger destination changes nothing
        assert e2 == 0 and bytes(o2) == expected
        if len(expected):
            assert model_decode(oracle, frame, len(expected) - 1)[0] != 0  # one byte short
    elif verdict == "invalid":
        assert ref_answer[0] != 0, "the reference accepts the near miss"
        assert model_answer is None, "the host model accepts what the reference rejects"
    elif verdict == "stricter":
        assert ref_answer == want  # (outside RFC 8878 as written, but the reference decodes it)
        assert model_answer is None  # stricter than the reference: allowed
    else:
        assert verdict == "checksum"
        assert ref_answer[0] != 0  # the reference verifies the content checksum,
        assert model_answer == want  # this library skips it (zstd_decode_core.h, "Not supported")


def test_near_miss_rows_have_their_frames():
    by_name = {c["name"]: c for c in F.CASES}
    for row, name in F.NEAR_MISSES.items():
        assert name in by_name and by_name[name]["verdict"] in ("invalid", "stricter"), f"near miss '{row}' has no frame"
    assert sum(c["verdict"] == "checksum" for c in F.CASES) == 1
    assert sorted(c["name"] for c in F.CASES if c["large"]) == ["every offset code up to 23, and a sequence of 80 bits", "offset value of 2^24 and more"]
    assert {c["path"] for c in F.CASES if c["verdict"] == "valid"} == {"parallel", "unlisted", "handed_back"}


# ---- the reference encoder's frames ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_census(oracle):
    """{setting: {feature: count}} over the reference encoder's frames of test_decoder_reads_reference_encoder_output's inputs:
    regenerated and compared with the committed summary where the reference is built, read from it elsewhere"""
    committed = json.loads(CENSUS_FILE.read_text()) if CENSUS_FILE.exists() else None
    if not have_ref():
        assert committed is not None, "tests/golden/zstd_ref_census.json is missing"
        return committed["settings"]
    from tests.test_zstd_model import reference_encoder_inputs

    r = get_ref()
    settings = {}
    for w in range(5):
        total = Counter()
        for d in reference_encoder_inputs(oracle, w):
            total += Z.census(bytes(r.compress(1, r.dll.refh_zstd_type(w), d)), seq_limit=SEQ_LIMIT)
        settings[str(w)] = dict(sorted(total.items()))
    fresh = dict(seq_limit=SEQ_LIMIT, settings=settings)
    if os.environ.get("LTHIP_RECORD_REF") == "1":
        CENSUS_FILE.write_text(json.dumps(fresh, indent=0, sort_keys=True) + "\n")
    else:
        assert committed == fresh, "the census of the reference frames changed: record it again (LTHIP_RECORD_REF=1)"
    return settings


# what the docstring of test_decoder_reads_reference_encoder_output claims, and the settings (0..4 = levels 3, 3, 22, 8, 22) at which the
# census finds it.  Everything claimed is there at some setting; Repeat_Mode and the second and third repeat offset only at the
# higher levels, an RLE offset table only at level 22.
CLAIMED = {
    "huf_direct": "01234", "huf_fse": "01234", "lit_treeless": "01234", "lit_huf_1stream": "01234", "lit_huf_4stream": "01234",
    "ll_predefined": "01234", "of_predefined": "01234", "ml_predefined": "01234", "ll_fse": "01234", "of_fse": "01234", "ml_fse": "01234",
    "ll_rle": "01234", "ml_rle": "01234", "of_rle": "24", "ll_repeat": "234", "of_repeat": "234", "ml_repeat": "234",
    "offset_value_1_ll": "01234", "offset_value_1_ll0": "01234", "offset_value_2_ll": "24", "offset_value_2_ll0": "24", "offset_value_3_ll": "24",
}
# legal forms the reference encoder's frames of these inputs do NOT contain (the crafted frames are their only test)
NOT_IN_REFERENCE_FRAMES = ["lit_rle", "repeat_after_predefined", "repeat_after_rle", "repeat_across_zero_seq_block", "repeat_across_raw_rle_block",
                           "nbseq_3byte", "offset_value_3_ll0", "raw_block_empty_mid", "checksum", "fcs_8", "concatenated", "skippable",
                           "offset_value_ge_2p24", "seq_bits_above_64", "huf_two_symbols", "huf_max_bits_11", "lit_huf_last_stream_empty",
                           "initial_history_4_used", "history_across_raw", "history_across_rle", "history_across_zero_seq"]


def test_reference_fixtures_contain_what_is_claimed(ref_census):
    for feature, where in CLAIMED.items():
        got = "".join(w for w in "01234" if ref_census[w].get(feature, 0))
        assert got == where, f"{feature}: found at settings '{got}', stated '{where}'"
    for feature in NOT_IN_REFERENCE_FRAMES:
        assert not any(ref_census[w].get(feature, 0) for w in "01234"), f"{feature} is in the reference's frames after all"


def test_every_feature_row_has_a_frame(ref_census):
    have = Counter()
    for c in F.CASES:
        if c["verdict"] == "valid":
            have += Z.census(F.built(c["name"])[0])
    crafted = set(have)
    for w in ref_census.values():
        have.update({k: v for k, v in w.items() if v})
    empty = [row for row in F.FEATURES if not have[row]]
    assert not empty, f"feature rows without a frame: {empty}"
    # FSE-coded Huffman weights are the one row the writer does not make: the reference's frames hold it (at every setting)
    assert [row for row in F.FEATURES if row not in crafted] == ["huf_fse"]
    for feature in NOT_IN_REFERENCE_FRAMES:
        assert feature in crafted, feature
