"""What the GPU tests of the zstd encoder share: a frame of k_zstd.hip taken apart into its 128 KiB pieces (the directory read against
the block headers), and the host model (oracle/zstd_model.c) run on the GPU match finder's own units, which must give every
Compressed piece byte for byte (tests/test_gpu_codecs.py, tests/test_gpu_zstd_encoder_sources.py)."""
import numpy as np


def zstd_pieces(frame: np.ndarray, versions=(2, 3)):
    """[(type, payload bytes)] per 128 KiB piece of a single-segment frame with an 8-byte content size (the layouts k_zstd.hip
    writes).  A piece is one block -- or, in frames that end with the "LTP\\2" directory, a run of sub-blocks (one per 4 KiB unit):
    then type 2 and the payload is the run WITH its block headers, Last_Block cleared (what zb_encode_piece_sub returns).
    versions: the directory versions the caller expects (4, the chained pieces of quality 2, only where it says so)."""
    assert bytes(frame[:5]) == bytes([0x28, 0xB5, 0x2F, 0xFD, 0xE0])
    content = int.from_bytes(bytes(frame[5:13]), "little")
    nunits = (content + 4095) // 4096
    pos, blocks = 13, []
    while True:
        h = int(frame[pos]) | int(frame[pos + 1]) << 8 | int(frame[pos + 2]) << 16
        last, typ, size = h & 1, (h >> 1) & 3, h >> 3
        n = 1 if typ == 1 else size
        blocks.append((typ, pos, 3 + n))
        pos += 3 + n
        if last:
            break
    tail = bytes(frame[pos:])
    magic = bytes([0x5D, 0x2A, 0x4D, 0x18])
    if tail[:4] == magic and tail[8:11] == b"LTP" and tail[11] in versions:
        # sub-block frames: skippable frame with the directory, one u16 per unit
        assert len(tail) == 12 + 2 * nunits and int.from_bytes(tail[4:8], "little") == 4 + 2 * nunits
        d = np.frombuffer(tail[12:], dtype="<u2")
        out, k = [], 0
        for u0 in range(0, nunits, 32):
            nu = min(32, nunits - u0)
            if d[u0] >= 0xFFFE:
                assert (d[u0 : u0 + nu] == d[u0]).all()
                typ, p0, n = blocks[k]
                assert typ == (0 if d[u0] == 0xFFFF else 1)
                out.append((typ, frame[p0 + 3 : p0 + n]))
                k += 1
            else:
                p0 = blocks[k][1]
                for u in range(nu):
                    typ, _, n = blocks[k + u]
                    assert n == 3 + (int(d[u0 + u]) & 0x7FFF) and typ == (0 if d[u0 + u] & 0x8000 else 2)
                end = blocks[k + nu - 1][1] + blocks[k + nu - 1][2]
                run = frame[p0:end].copy()
                run[blocks[k + nu - 1][1] - p0] &= 0xFE
                out.append((2, run))
                k += nu
        assert k == len(blocks)
        return out
    # frames of two or more pieces end with the independence marker: a skippable frame (k_zstd.hip z_write_trailer)
    if tail:
        assert len(blocks) >= 2 and tail == magic + bytes([4, 0, 0, 0]) + b"LTP\x01"
    return [(typ, frame[p0 + 3 : p0 + n]) for typ, p0, n in blocks]


def model_src(oracle):
    import ctypes as C

    d = oracle.dll
    d.ltz_model_encode_block_src.restype = C.c_uint32
    d.ltz_model_encode_block_src.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return d


def model_compress(oracle, b: np.ndarray) -> np.ndarray:
    """the host model's frame of b, with its own greedy matcher (ltz_model_compress)"""
    import ctypes as C

    d = oracle.dll
    d.ltz_model_bound.restype = C.c_size_t
    d.ltz_model_bound.argtypes = [C.c_size_t]
    d.ltz_model_compress.restype = C.c_int
    d.ltz_model_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    b = np.ascontiguousarray(b, dtype=np.uint8)
    cap = d.ltz_model_bound(len(b))
    out = np.zeros(cap + 8, np.uint8)
    n = C.c_size_t(0)
    assert d.ltz_model_compress(b.ctypes.data, len(b), out.ctypes.data, cap, C.byref(n)) == 0
    return out[: n.value].copy()


def check_against_model(gpu, d, blocks, frames):
    """every Compressed_Block of `frames` == the host model run on the GPU match finder's units; Raw where the model says so"""
    unit0 = 0
    checked = 0
    for b, f in zip(blocks, frames):
        b = np.ascontiguousarray(b)
        nunits = (len(b) + 4095) // 4096
        meta, lits, recs = gpu.zstd_debug_units(unit0, nunits)
        for i, (typ, payload) in enumerate(zstd_pieces(f)):
            raw = min(131072, len(b) - i * 131072)
            nu = (raw + 4095) // 4096
            out = np.zeros(140000, np.uint8)
            m, l, r = (np.ascontiguousarray(a[i * 32 : i * 32 + nu]) for a in (meta, lits, recs))
            l[m[:, 0] == 0] = 0x5A  # units without a sequence have no literal buffer: their literals are the source bytes
            piece = b[i * 131072 : i * 131072 + raw]
            n = d.ltz_model_encode_block_src(m.ctypes.data, l.ctypes.data, r.ctypes.data, nu, raw, piece.ctypes.data, out.ctypes.data)
            if typ == 2:
                assert n == len(payload) and (out[:n] == payload).all()
                checked += 1
            elif typ == 0:
                assert n == 0
        unit0 += nunits
    return checked
