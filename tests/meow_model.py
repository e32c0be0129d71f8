"""A CPU model of Meow hash v0.5 as longtail's 'meow' hash type uses it (MeowBegin / MeowAbsorb / MeowEnd with the default seed, the
digest = the low 64 bits of the 128-bit result), written from the algorithm's description and FIPS-197.  It checks the GPU kernels
(tests/test_gpu_meow.py) and backs a Python Longtail_HashAPI for the reference core.

State: eight 128-bit registers, each held as four little-endian 32-bit columns (the AES state's columns: byte i at row i % 4,
column i // 4).  aesdec(a, k) = InvMixColumns(InvSubBytes(InvShiftRows(a))) ^ k, computed with one word table TD (InvSubBytes and
InvMixColumns of a byte in row 0) and its byte rotations for rows 1..3.  paddq adds the 64-bit halves (columns 0,1 and 2,3).

The functions take a batch of messages as a zero-padded uint8 matrix and a length per row, so that many messages are hashed at once."""
import numpy as np

M64 = (1 << 64) - 1


# ---- π in hexadecimal: the default seed is its first 256 hex digits, the leading "3" included ----
def pi_hex_digits(n: int) -> str:
    """The first n hexadecimal digits of π (Machin: π = 16 atan(1/5) - 4 atan(1/239)), in fixed point with guard bits."""
    bits = 4 * n + 64
    one = 1 << bits

    def atan_inv(x: int) -> int:
        total, term, k, sign = 0, one // x, 1, 1
        x2 = x * x
        while term:
            total += sign * (term // k)
            term //= x2
            k += 2
            sign = -sign
        return total

    pi = 16 * atan_inv(5) - 4 * atan_inv(239)
    return format(pi >> (bits - 4 * (n - 1)), "X")[:n]


SEED = bytes.fromhex(pi_hex_digits(256))


# ---- AES decryption round tables from FIPS-197 ----
def _gmul(a: int, b: int) -> int:
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = ((a << 1) ^ 0x11B) if a & 0x80 else a << 1
        b >>= 1
    return r


def _sbox():
    inv = [0] * 256
    for x in range(1, 256):
        for y in range(1, 256):
            if _gmul(x, y) == 1:
                inv[x] = y
                break
    s = []
    for x in range(256):
        b = inv[x]
        v = b
        for k in (1, 2, 3, 4):
            v ^= ((b << k) | (b >> (8 - k))) & 0xFF
        s.append(v ^ 0x63)
    return s


SBOX = _sbox()
INV_SBOX = [0] * 256
for _x, _y in enumerate(SBOX):
    INV_SBOX[_y] = _x
# InvMixColumns column of a byte s in row 0: (0e s, 09 s, 0d s, 0b s) as a little-endian word; rows 1..3 are byte rotations of it
TD = np.array([_gmul(s, 0x0E) | _gmul(s, 0x09) << 8 | _gmul(s, 0x0D) << 16 | _gmul(s, 0x0B) << 24 for s in INV_SBOX], np.uint32)


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def aesdec(a, k):
    """a, k: (..., 4) uint32 columns"""
    b0 = TD[a & 0xFF]
    b1 = _rotl(TD[(np.roll(a, 1, axis=-1) >> 8) & 0xFF], 8)  # row 1 of column c comes from column c - 1 (InvShiftRows)
    b2 = _rotl(TD[(np.roll(a, 2, axis=-1) >> 16) & 0xFF], 16)
    b3 = _rotl(TD[np.roll(a, 3, axis=-1) >> 24], 24)
    return b0 ^ b1 ^ b2 ^ b3 ^ k


def paddq(a, b):
    return (a.view(np.uint64) + b.view(np.uint64)).view(np.uint32)


def _mix_reg(x, r1, r2, r3, r4, r5, i1, i2, i3, i4, act):
    """MEOW_MIX_REG on registers x[:, r] for the rows where act is set"""
    n = x.copy()
    n[:, r1] = aesdec(x[:, r1], x[:, r2])
    n[:, r3] = paddq(x[:, r3], i1)
    t = x[:, r2] ^ i2
    n[:, r2] = aesdec(t, x[:, r4])
    n[:, r5] = paddq(x[:, r5], i3)
    n[:, r4] = x[:, r4] ^ i4
    x[act] = n[act]


def _reg(lane, off):
    """16 bytes from byte `off` of each row's 32-byte lane, cyclically, as (N, 4) uint32"""
    idx = (np.arange(16) + off) % 32
    return np.ascontiguousarray(lane[:, idx]).view("<u4")


def _mix(x, j, lane, act):
    """MEOW_MIX with the register roles of lane j (mod 8) on a 32-byte lane: inputs at +15, +0, +1, +16"""
    _mix_reg(x, j % 8, (j + 4) % 8, (j + 6) % 8, (j + 1) % 8, (j + 2) % 8, _reg(lane, 15), _reg(lane, 0), _reg(lane, 1), _reg(lane, 16), act)


def _shuffle(x, i):
    r1, r2, r3, r4, r5, r6 = [(i + k) % 8 for k in (0, 1, 2, 4, 5, 6)]
    x[:, r1] = aesdec(x[:, r1], x[:, r4])
    x[:, r2] = paddq(x[:, r2], x[:, r5])
    x[:, r4] = x[:, r4] ^ x[:, r6]
    x[:, r4] = aesdec(x[:, r4], x[:, r2])
    x[:, r5] = paddq(x[:, r5], x[:, r6])
    x[:, r2] = x[:, r2] ^ x[:, r3]


def meow_batch(data, lens):
    """data: (N, W) uint8, row r's message in data[r, :lens[r]] (bytes past it are ignored); returns (N,) uint64 digests"""
    lens = np.asarray(lens, np.int64)
    n = len(lens)
    width = int(lens.max()) if n else 0
    pad = np.zeros((n, ((width >> 8) + 1) * 256 + 32), np.uint8)
    for r in range(n):
        pad[r, : lens[r]] = data[r, : lens[r]]
    x = np.tile(np.frombuffer(SEED, np.uint32).reshape(1, 8, 4), (n, 1, 1)).copy()
    blocks = lens >> 8
    for b in range(int(blocks.max()) if n else 0):
        act = blocks > b
        for j in range(8):
            _mix(x, j, pad[:, b * 256 + 32 * j : b * 256 + 32 * j + 32], act)
    # MeowEnd: R = the residual (< 256 bytes, zero beyond the message)
    rows = np.arange(n)[:, None]
    res = pad[rows, (blocks * 256)[:, None] + np.arange(256 + 32)[None, :]]
    res[np.arange(256 + 32)[None, :] >= (lens & 0xFF)[:, None]] = 0
    all_rows = np.ones(n, bool)
    # the tail lane: the last (Len & 31) bytes at Len & 0xe0, zero-padded to 32; inputs at cyclic offsets 31, 0, 17, 16
    tail = res[rows, ((lens & 0xE0))[:, None] + np.arange(32)[None, :]]
    _mix_reg(x, 0, 4, 6, 1, 2, _reg(tail, 31), _reg(tail, 0), _reg(tail, 17), _reg(tail, 16), all_rows)
    # the length: i3 = Len >> 8, i4 = Len (64-bit values in the low half), i1 = i2 = 0
    ln = np.zeros((n, 4), np.uint32)
    ln.view(np.uint64)[:, 0] = lens.astype(np.uint64)
    l8 = np.zeros((n, 4), np.uint32)
    l8.view(np.uint64)[:, 0] = (lens >> 8).astype(np.uint64)
    z = np.zeros((n, 4), np.uint32)
    _mix_reg(x, 1, 5, 7, 2, 3, z, z, l8, ln, all_rows)
    lanes = (lens >> 5) & 7
    for k in range(7):
        _mix(x, k + 2, res[:, 32 * k : 32 * k + 32], lanes > k)
    for i in range(12):
        _shuffle(x, i % 8)
    x0 = paddq(x[:, 0], x[:, 2])
    x1 = paddq(x[:, 1], x[:, 3])
    x4 = paddq(x[:, 4], x[:, 6])
    x5 = paddq(x[:, 5], x[:, 7])
    out = paddq(np.ascontiguousarray(x0 ^ x1), np.ascontiguousarray(x4 ^ x5))
    return np.ascontiguousarray(out).view(np.uint64)[:, 0].copy()


def meow(data) -> int:
    """The 'meow' digest of one message (bytes or a uint8 array)"""
    a = np.frombuffer(bytes(data), np.uint8)
    return int(meow_batch(a.reshape(1, -1), [len(a)])[0])


def meow_ranges(host, offsets, lens) -> np.ndarray:
    """Digests of the ranges host[o : o + n]: gathered into one padded matrix (ranges of similar length belong in one call)"""
    lens = np.asarray(lens, np.int64)
    offsets = np.asarray(offsets, np.int64)
    if len(lens) == 0:
        return np.zeros(0, np.uint64)
    w = max(1, int(lens.max()))
    m = np.zeros((len(lens), w), np.uint8)
    for r, (o, k) in enumerate(zip(offsets, lens)):
        m[r, :k] = host[o : o + k]
    return meow_batch(m, lens)


class MeowStream:
    """Streaming use (BeginContext / Hash / EndContext): Meow's absorb step is split-invariant, so the stream is its bytes"""

    def __init__(self):
        self.parts = []

    def update(self, b: bytes):
        self.parts.append(bytes(b))

    def digest(self) -> int:
        return meow(b"".join(self.parts))
