"""TEST INFRASTRUCTURE: the dropout stream of emo-disentanger_amd/csrc/emo_common.h restated in plain NumPy, from the header's comments and
formulas (make_drop, emo_hash32, emo_drop_hash, emo_xs32, drop_mult) — the project's own specification, held outside the library so that the
library's stream can be compared with it (tests/test_gpu_dropmask.py) and its statistics asserted without a GPU (tests/test_dropmask_host.py).

The stream: one keyed 32-bit hash per FOUR consecutive elements.  For the linear element index idx,
    quad = low32(idx >> 2) ^ low32(low32(idx >> 34) * 0x9E3779B1)            (the high-word fold: indices past 2^34)
    h    = emo_drop_hash(key, key2, quad);   if idx & 2: h = xorshift32(h)
    bits = idx & 1 ? h >> 16 : h & 0xFFFF;   keep iff bits >= thr16,   thr16 = (uint32)(p * 65536.f + 0.5f) in float32
and the multiplier of a kept element is float32(1) / (float32(1) - float32(p)).

All arithmetic is uint64 masked to 32 bits (NumPy's uint32 multiply would wrap the same way but warns on scalars)."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _u(x):
    return np.asarray(x, dtype=np.uint64) & _M32


def _mul(a, b):
    return (_u(a) * np.uint64(b)) & _M32


def hash32(x):
    """emo_hash32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16."""
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = _mul(x, 0x7FEB352D)
    x = x ^ (x >> np.uint64(15))
    x = _mul(x, 0x846CA68B)
    x = x ^ (x >> np.uint64(16))
    return x


def drop_hash(key, key2, pair):
    """emo_drop_hash: the counter enters un-multiplied, key before the first round, key2 between the two multiply rounds."""
    x = _u(pair) ^ np.uint64(key)
    x = x ^ (x >> np.uint64(16))
    x = _mul(x, 0x7FEB352D)
    x = x ^ np.uint64(key2)
    x = x ^ (x >> np.uint64(15))
    x = _mul(x, 0x846CA68B)
    x = x ^ (x >> np.uint64(16))
    return x


def xs32(x):
    """emo_xs32: x ^= x << 13; x ^= x >> 17; x ^= x << 5 (32-bit)."""
    x = _u(x)
    x = x ^ ((x << np.uint64(13)) & _M32)
    x = x ^ (x >> np.uint64(17))
    x = x ^ ((x << np.uint64(5)) & _M32)
    return x


def make_drop(p, seed, offset):
    """(key, key2, thr16, scale) of the stream (p, seed, offset): key / key2 / thr16 Python ints, scale a numpy float32.  p is taken as the C
    float the library receives; thr16 and scale are float32 arithmetic as in the header; thr16 == 0 means dropout off."""
    p32 = np.float32(p)
    if p32 > np.float32(0):
        thr16 = int(np.uint32(p32 * np.float32(65536.0) + np.float32(0.5)))
        scale = np.float32(1.0) / (np.float32(1.0) - p32)
    else:
        thr16, scale = 0, np.float32(1.0)
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    s0, s1, o0, o1 = seed & 0xFFFFFFFF, seed >> 32, offset & 0xFFFFFFFF, offset >> 32
    k = int(hash32(s0 ^ 0x9E3779B9))
    k = int(hash32(k ^ s1))
    k = int(hash32(k ^ int(_mul(o0, 0x85EBCA6B)) ^ o1))               # (* binds tighter than ^ in the header's expression)
    k2 = int(hash32(s1 ^ 0xC2B2AE35))
    k2 = int(hash32((k2 + o0) & 0xFFFFFFFF))
    k2 = int(hash32(k2 ^ int(_mul(s0, 0x27D4EB2F)) ^ int(_mul(o1, 0x165667B1))))
    return k, k2, thr16, scale


def keep_at(idx, p, seed, offset):
    """bool keep decisions of the linear element indices `idx` (any integer array, values < 2^64)."""
    idx = np.asarray(idx, dtype=np.uint64)
    key, key2, thr16, _ = make_drop(p, seed, offset)
    if thr16 == 0:
        return np.ones(idx.shape, dtype=bool)
    quad = ((idx >> np.uint64(2)) & _M32) ^ _mul(idx >> np.uint64(34), 0x9E3779B1)
    h = drop_hash(key, key2, quad)
    h = np.where((idx & np.uint64(2)) != 0, xs32(h), h)
    bits = np.where((idx & np.uint64(1)) != 0, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return bits >= np.uint64(thr16)


def keep(n, p, seed, offset, start=0):
    """bool[n]: keep decisions of the linear element indices start .. start + n - 1."""
    return keep_at(np.uint64(start) + np.arange(n, dtype=np.uint64), p, seed, offset)


def multipliers(shape, p, seed, offset, start=0):
    """float32[shape]: keep * float32(1 / (1 - p)) of a contiguous tensor whose first element has linear index `start`."""
    n = int(np.prod(shape))
    scale = make_drop(p, seed, offset)[3]
    return (keep(n, p, seed, offset, start).astype(np.float32) * scale).reshape(shape)
