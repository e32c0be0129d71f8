"""CPU-only checks of the in-place update interface (include/longtail_hip.h, "updating a resident version in place"): the four entry points
are declared and exported by both builds, the code object holds the new kernels, the package exports the new names, the device entries
refuse null arguments, and lthip_restore_layout_in_place gives the offsets of a Python model of its rule on versions built by hand.  Every
comparison is equality."""
import ctypes as C
import errno
import subprocess

import numpy as np
import pytest

from tests.restore_util import BLK2, BLK3
from tests.test_abi import declared_symbols
from tests.update_util import build_version_index

NEW_SYMBOLS = ["lthip_restore_layout_in_place", "lthip_restore_in_place_scratch_bound", "lthip_restore_in_place_stats",
               "lthip_restore_carry_in_place"]
KERNELS = ["k_restore_in_place_classify", "k_restore_in_place_slots"]
SKIP = 0xFFFFFFFFFFFFFFFF


def version(assets, hash_id=BLK3):
    """assets: (name, path hash, content hash, size); one chunk per file of size > 0 (its content hash names it)."""
    files = [a for a in assets if a[3]]
    chunk_of = {a[0]: k for k, a in enumerate(files)}
    return build_version_index(hash_id, 32768, [a[0] for a in assets], [[chunk_of[a[0]]] if a[3] else [] for a in assets],
                               [a[2] for a in files], [a[3] for a in files], path_hashes=[a[1] for a in assets],
                               content_hashes=[a[2] for a in assets])


def model(base, base_offsets, base_bytes, target, align):
    """The rule of lthip_restore_layout_in_place -> (offsets, total bytes, kept assets)."""
    up = lambda x: (x + align - 1) // align * align
    resident = {a[1]: (a, o) for a, o in zip(base, base_offsets) if o != SKIP}
    kept = {k: resident[t[1]][1] for k, t in enumerate(target)
            if t[3] and t[1] in resident and resident[t[1]][0][2:] == t[2:]}
    gaps, at = [], 0
    for o, n in sorted((o, target[k][3]) for k, o in kept.items()):
        if o > at:
            gaps.append([at, o])
        at = o + n
    if base_bytes > at:
        gaps.append([at, base_bytes])
    offsets, end = [], base_bytes
    for k, t in enumerate(target):
        if not t[3]:
            offsets.append(0)
        elif k in kept:
            offsets.append(kept[k])
        else:
            g = next((g for g in gaps if up(g[0]) + t[3] <= g[1]), None)
            if g:
                offsets.append(up(g[0]))
                g[0] = offsets[-1] + t[3]
            else:
                offsets.append(up(end))
                end = offsets[-1] + t[3]
    return offsets, max([o + t[3] for o, t in zip(offsets, target) if t[3]], default=0), len(kept)


def layout(dll, base_vi, base_offsets, base_bytes, target_vi, align, n_target, offsets=True):
    a, b = np.frombuffer(base_vi, np.uint8), np.frombuffer(target_vi, np.uint8)
    bo = np.array(list(base_offsets) + [0], np.uint64)
    out = np.full(max(n_target, 1), 0xDEAD, np.uint64)
    count, total, kept = C.c_uint32(0xDEAD), C.c_uint64(0xDEAD), C.c_uint32(0xDEAD)
    err = dll.lthip_restore_layout_in_place(a.ctypes.data, len(a), bo.ctypes.data, base_bytes, b.ctypes.data, len(b), align,
                                            out.ctypes.data if offsets else None, C.byref(count), C.byref(total), C.byref(kept))
    return err, out[:n_target].tolist(), count.value, total.value, kept.value


# (name, path hash, content hash, size); the base lies dense at 16-byte boundaries unless a case says otherwise
BASE = [("dir/", 90, 0, 0), ("a.bin", 30, 1001, 1000), ("b.bin", 10, 1002, 5000), ("c.bin", 50, 1003, 300), ("d.bin", 20, 1004, 2500),
        ("empty", 70, 0, 0), ("e.bin", 40, 1005, 64)]


def dense(assets, align=16, skip=()):
    offs, at = [], 0
    for k, a in enumerate(assets):
        at = (at + align - 1) // align * align
        offs.append(SKIP if k in skip else at)
        at += a[3]
    return offs, at


def changed(**new):
    """BASE with assets replaced by name: name=(content hash, size), or None to remove it."""
    out = []
    for a in BASE:
        if a[0] in new and new[a[0]] is None:
            continue
        out.append((a[0], a[1]) + tuple(new[a[0]]) if a[0] in new else a)
    return out


CASES = {
    "everything kept": dict(target=list(reversed(BASE))),
    "nothing kept": dict(target=[(a[0], a[1], a[2] + 7 if a[3] else 0, a[3]) for a in BASE]),
    # b.bin shrinks and fits its own old gap; d.bin grows, fits no gap and is appended
    "modified: one fits its gap, one is appended": dict(target=changed(**{"b.bin": (2002, 4000), "d.bin": (2004, 9000)})),
    # b.bin (5000 bytes) is gone; two added assets share its gap, a third does not fit any more
    "a removed asset's gap takes two added ones": dict(
        target=changed(**{"b.bin": None}) + [("n1.bin", 61, 3001, 2000), ("n2.bin", 62, 3002, 2900), ("n3.bin", 63, 3003, 200)]),
    "a base asset that is not resident": dict(target=list(BASE), skip=(2,)),
    "the total lies below the base": dict(target=changed(**{"e.bin": None, "d.bin": None})),
    "same path and content, another size": dict(target=changed(**{"c.bin": (1003, 301)})),
}


@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("case", list(CASES))
def test_layout_in_place_is_the_model(hiplib, case, align):
    c = CASES[case]
    target = c["target"]
    base_offsets, base_bytes = dense(BASE, skip=c.get("skip", ()))
    want = model(BASE, base_offsets, base_bytes, target, align)
    err, offsets, count, total, kept = layout(hiplib.dll, version(BASE), base_offsets, base_bytes, version(target), align, len(target))
    assert err == 0
    assert (offsets, total, kept) == want and count == len(target)
    err, _, count, total, kept = layout(hiplib.dll, version(BASE), base_offsets, base_bytes, version(target), align, len(target), offsets=False)
    assert err == 0 and (count, total, kept) == (len(target), want[1], want[2])
    from longtail_amd.lib import restore_layout_in_place

    got = restore_layout_in_place(version(BASE), base_offsets, base_bytes, version(target), align, hiplib)
    assert (got[0].tolist(), got[1], got[2]) == want
    # the windows of the assets with bytes are disjoint, and a kept asset lies where the base has it
    spans = sorted((o, o + t[3]) for o, t in zip(offsets, target) if t[3])
    assert all(p[1] <= q[0] for p, q in zip(spans, spans[1:]))


def test_the_cases_hold_what_they_should():
    """Written out by hand for align 16, so that the model itself is pinned."""
    base_offsets, base_bytes = dense(BASE)
    assert (base_offsets, base_bytes) == ([0, 0, 1008, 6016, 6320, 8832, 8832], 8896)
    m = lambda case, align=16: model(BASE, dense(BASE, skip=CASES[case].get("skip", ()))[0], base_bytes, CASES[case]["target"], align)
    assert m("everything kept") == ([8832, 0, 6320, 6016, 1008, 0, 0], 8896, 5)
    assert m("nothing kept") == ([0, 0, 1008, 6016, 6320, 0, 8832], 8896, 0)  # one gap, filled in asset order
    # kept: a, c, e.  gaps: [1000, 6016) [6316, 8832).  b (4000) -> 1008; d (9000) fits neither -> appended at 8896
    assert m("modified: one fits its gap, one is appended") == ([0, 0, 1008, 6016, 8896, 0, 8832], 17896, 3)
    # gaps: [1000, 6016) [6316, 6320) [8820, 8832).  n1 -> 1008, n2 -> 3008 (ends 5908), n3 (200) fits nothing -> appended
    assert m("a removed asset's gap takes two added ones") == ([0, 0, 6016, 6320, 0, 8832, 1008, 3008, 8896], 9096, 4)
    # b is not resident: its window [1000, 6016) is a gap, and the target's b goes there
    assert m("a base asset that is not resident") == ([0, 0, 1008, 6016, 6320, 0, 8832], 8896, 4)
    assert m("the total lies below the base") == ([0, 0, 1008, 6016, 0], 6316, 3)
    # c grows by a byte: not kept; its old gap [6016, 6320) still holds it at align 16, but not at 4096
    assert m("same path and content, another size")[0][3] == 6016 and m("same path and content, another size", 4096)[0][3] == 12288


def test_layout_in_place_refusals(hiplib):
    base_offsets, base_bytes = dense(BASE)
    a, b = version(BASE), version(CASES["nothing kept"]["target"])
    dll, n = hiplib.dll, len(BASE)
    lay = lambda *args, **kw: layout(dll, *args, **kw)[0]
    assert lay(a, base_offsets, base_bytes, b, 16, n) == 0
    # ---- EBADF ----
    assert lay(a[:-1], base_offsets, base_bytes, b, 16, n) == errno.EBADF  # truncated: the last path loses its terminator
    assert lay(a, base_offsets, base_bytes, b[:40], 16, n) == errno.EBADF
    twice = [list(x) for x in BASE]
    twice[3][1] = twice[1][1]  # two assets of one version with the same path hash
    assert lay(version([tuple(x) for x in twice]), base_offsets, base_bytes, b, 16, n) == errno.EBADF
    assert lay(a, base_offsets, base_bytes, version([tuple(x) for x in twice]), 16, n) == errno.EBADF
    # ---- EINVAL ----
    for align in (0, 3, 24):
        assert lay(a, base_offsets, base_bytes, b, align, n) == errno.EINVAL
    ra, rb = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    bo = np.array(base_offsets, np.uint64)
    total = C.c_uint64(0)
    args = lambda pa, pb, po: (pa, len(ra), po, base_bytes, pb, len(rb), 16, None, None, C.byref(total), None)
    assert dll.lthip_restore_layout_in_place(*args(ra.ctypes.data, rb.ctypes.data, bo.ctypes.data)) == 0 and total.value == base_bytes
    assert dll.lthip_restore_layout_in_place(*args(None, rb.ctypes.data, bo.ctypes.data)) == errno.EINVAL
    assert dll.lthip_restore_layout_in_place(*args(ra.ctypes.data, None, bo.ctypes.data)) == errno.EINVAL
    assert dll.lthip_restore_layout_in_place(*args(ra.ctypes.data, rb.ctypes.data, None)) == errno.EINVAL
    assert lay(a, base_offsets, base_bytes, version(CASES["nothing kept"]["target"], BLK2), 16, n) == errno.EINVAL  # hash identifiers differ
    assert lay(a, base_offsets, base_bytes - 1, b, 16, n) == errno.EINVAL  # the last resident asset leaves [0, base_bytes)
    outside = list(base_offsets)
    outside[1] = base_bytes + 1
    assert lay(a, outside, base_bytes, b, 16, n) == errno.EINVAL
    overlap = list(base_offsets)
    overlap[2] = 999  # b.bin starts inside a.bin: both are kept by an unchanged target
    assert lay(a, overlap, base_bytes, a, 16, n) == errno.EINVAL
    assert lay(a, overlap, base_bytes, b, 16, n) == 0  # ... and nothing overlaps when neither is kept


def test_entry_points_are_declared_and_exported(hiplib):
    assert set(NEW_SYMBOLS) <= set(declared_symbols())
    assert not [n for n in NEW_SYMBOLS if not hasattr(hiplib.dll, n)]
    from longtail_amd.lib import ABLATIONS_LIB_PATH

    if ABLATIONS_LIB_PATH.exists():
        abl = C.CDLL(str(ABLATIONS_LIB_PATH))
        assert not [n for n in NEW_SYMBOLS if not hasattr(abl, n)]
    assert hiplib.dll.lthip_abi_version() == 4


def test_code_object_holds_the_in_place_kernels(hiplib):
    text = subprocess.run(["strings", "-a", str(hiplib.path)], capture_output=True, text=True, check=True).stdout
    for k in KERNELS:
        assert k in text, k


def test_the_package_exports_the_new_names():
    import longtail_amd
    from longtail_amd.lib import Restore, restore_layout_in_place

    assert longtail_amd.restore_layout_in_place is restore_layout_in_place
    assert callable(Restore.carry_in_place) and callable(Restore.in_place_stats) and callable(Restore.in_place_scratch_bound)


def test_the_session_entries_refuse_null_arguments(hiplib):
    dll = hiplib.dll
    out = np.full(4, 7, np.uint64)
    assert dll.lthip_restore_carry_in_place(None, None, None, 0) == errno.EINVAL
    assert dll.lthip_restore_in_place_stats(None, out.ctypes.data) == errno.EINVAL and out.tolist() == [7] * 4
    assert dll.lthip_restore_in_place_scratch_bound(None) == 0
