"""Host tests of tests/dropmask_ref.py, the NumPy restatement of the dropout stream that emo-disentanger_amd/csrc/emo_common.h specifies, and of
the stream's statistics (no GPU: tests/test_gpu_dropmask.py pins the library's kernels to this port bit for bit, so what is asserted here about
the port holds for the kernels).

Every statistic is asserted within 5 sigma of its expectation under independent Bernoulli(keep) draws: the binomial sigma for a rate, 1 / sqrt(n)
for a correlation coefficient.  The inputs are fixed, so the results are deterministic; the 5-sigma cap is a condition on the stream, not a
measurement (a truly random stream exceeds it once in 1.7 million statistics).  Worst observed |z| on this file's 534 statistics: 3.8
(p = 0.1: 3.3, p = 0.25: 2.6, p = 0.5: 3.8)."""
import math

import numpy as np
import pytest

import dropmask_ref as R

M32 = 0xFFFFFFFF
SEED = 12345
LAGS = (1, 2, 3, 4, 8, 64, 512, 2048)
# the engine's per-site offsets (engine.py: layer l = base + 8 (l + 1) + {1, 2, 3}; base = 4096 per forward)
SITE_OFFSETS = [base + 8 * (l + 1) + k for base in (4096, 8192) for l in (0, 1) for k in (1, 2, 3)]


# ---------------------------------------------------------------------------------------------------- one element in pure Python ints
def _h32(x):
    x ^= x >> 16; x = x * 0x7FEB352D & M32; x ^= x >> 15; x = x * 0x846CA68B & M32; x ^= x >> 16
    return x


def scalar_keep(idx, p, seed, offset):
    """drop_mult() of emo_common.h for ONE element, Python integers only (an independent second writing of the port)."""
    p32 = np.float32(p)
    if not p32 > 0:
        return True
    thr16 = int(p32 * np.float32(65536.0) + np.float32(0.5))
    s0, s1, o0, o1 = seed & M32, (seed >> 32) & M32, offset & M32, (offset >> 32) & M32
    k = _h32(s0 ^ 0x9E3779B9)
    k = _h32(k ^ s1)
    k = _h32(k ^ (o0 * 0x85EBCA6B & M32) ^ o1)
    k2 = _h32(s1 ^ 0xC2B2AE35)
    k2 = _h32((k2 + o0) & M32)
    k2 = _h32(k2 ^ (s0 * 0x27D4EB2F & M32) ^ (o1 * 0x165667B1 & M32))
    quad = ((idx >> 2) & M32) ^ (((idx >> 34) & M32) * 0x9E3779B1 & M32)
    x = quad ^ k
    x ^= x >> 16; x = x * 0x7FEB352D & M32; x ^= k2; x ^= x >> 15; x = x * 0x846CA68B & M32; x ^= x >> 16
    if idx & 2:
        x ^= x << 13 & M32; x ^= x >> 17; x ^= x << 5 & M32
    bits = x >> 16 if idx & 1 else x & 0xFFFF
    return bits >= thr16


def test_scalar_and_vectorised_agree():
    rng = np.random.default_rng(0)
    idx = np.concatenate([rng.integers(0, 2 ** 20, 1024), rng.integers(0, 2 ** 34, 1024), rng.integers(2 ** 34, 2 ** 40, 1024),
                          rng.integers(2 ** 40, 2 ** 62, 1020), np.array([2 ** 34, 2 ** 34 + 1, 2 ** 34 + 2, 2 ** 34 + 3])]).astype(np.uint64)
    assert idx.size == 4096 and (idx >= 2 ** 34).sum() >= 2048
    assert all(((idx & np.uint64(3)) == np.uint64(r)).sum() > 900 for r in range(4))          # all four fields of a hash
    for p, seed, offset in ((0.1, SEED, 4105), (0.25, (7 << 32) | 99, (3 << 32) | 4106), (0.5, 2 ** 64 - 1, 2 ** 64 - 1)):
        vec = R.keep_at(idx, p, seed, offset)
        ref = np.array([scalar_keep(int(i), p, seed, offset) for i in idx])
        assert np.array_equal(vec, ref), (p, seed, offset, int((vec != ref).sum()))
        assert 0 < vec.sum() < vec.size
    # keep() is keep_at() of a range, the fold included
    assert np.array_equal(R.keep(64, 0.1, SEED, 7, start=2 ** 34 - 32), R.keep_at(np.arange(2 ** 34 - 32, 2 ** 34 + 32, dtype=np.uint64), 0.1, SEED, 7))


def test_p_zero_is_all_ones():
    assert R.make_drop(0.0, SEED, 5)[2:] == (0, np.float32(1.0))
    assert R.keep(4096, 0.0, SEED, 5).all()
    m = R.multipliers((8, 16), 0.0, SEED, 5)
    assert m.dtype == np.float32 and m.shape == (8, 16) and (m == 1.0).all()


@pytest.mark.parametrize('p, thr16', [(0.1, 6554), (0.25, 16384), (0.5, 32768), (1.0 / 65536, 1)])
def test_thr16_and_scale(p, thr16):
    # 0.1f = 0.100000001490116..., * 65536 = 6553.6001 (fp32: 6553.60009765625), + 0.5 -> 6554.1 -> 6554
    key, key2, t, scale = R.make_drop(p, SEED, 0)
    assert t == thr16
    assert scale.dtype == np.float32 and scale == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert 0 <= key <= M32 and 0 <= key2 <= M32
    m = R.multipliers((1024,), p, SEED, 0)
    assert set(np.unique(m).tolist()) <= {0.0, float(scale)}


def _z_disagree(a, b, keep_rate):
    q = 2.0 * keep_rate * (1.0 - keep_rate)
    return ((a != b).mean() - q) / math.sqrt(q * (1.0 - q) / a.size)


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_every_key_word_changes_the_stream(p):
    """Streams whose seeds / offsets differ ONLY in the high word, or by one, are different streams: they disagree at the share of positions that
    two independent Bernoulli(keep) masks disagree at, 2 keep (1 - keep), within 5 sigma."""
    n = 1 << 20
    kr = 1.0 - R.make_drop(p, 0, 0)[2] / 65536.0
    base = R.keep(n, p, SEED, 4105)
    zs = {'seed hi': _z_disagree(base, R.keep(n, p, SEED | (1 << 32), 4105), kr),
          'seed hi 2': _z_disagree(R.keep(n, p, SEED | (1 << 32), 4105), R.keep(n, p, SEED | (2 << 32), 4105), kr),
          'offset hi': _z_disagree(base, R.keep(n, p, SEED, 4105 | (1 << 32)), kr),
          'offset hi 2': _z_disagree(R.keep(n, p, SEED, 4105 | (1 << 32)), R.keep(n, p, SEED, 4105 | (1 << 63)), kr),
          'seed + 1': _z_disagree(base, R.keep(n, p, SEED + 1, 4105), kr),
          'offset + 1': _z_disagree(base, R.keep(n, p, SEED, 4106), kr)}
    print(zs)
    assert all(abs(z) <= 5.0 for z in zs.values()), zs


def _stream_z(p, n):
    """|z| of every statistic of the engine's twelve site streams at (p, n): name -> z."""
    kr = 1.0 - R.make_drop(p, SEED, 0)[2] / 65536.0
    var = kr * (1.0 - kr)
    xs, z = [], {}
    for off in SITE_OFFSETS:
        k = R.keep(n, p, SEED, off)
        z['rate@%d' % off] = (k.mean() - kr) / math.sqrt(var / n)
        xs.append(k.astype(np.float32) - np.float32(kr))
    for off, x in zip(SITE_OFFSETS, xs):
        for lag in LAGS:
            z['lag%d@%d' % (lag, off)] = float(np.dot(x[:-lag], x[lag:], ) / (n - lag) / var) * math.sqrt(n)
    for i in range(len(xs)):
        for j in range(i + 1, len(xs)):
            z['cross@%d,%d' % (SITE_OFFSETS[i], SITE_OFFSETS[j])] = float(np.dot(xs[i], xs[j]) / n / var) * math.sqrt(n)
    return z


@pytest.mark.parametrize('p, log2n', [(0.1, 22), (0.25, 20), (0.5, 20)])
def test_stream_statistics_within_5_sigma(p, log2n):
    """Keep rate of every site stream against 1 - thr16 / 65536, serial correlation at LAGS, every pairwise cross-stream correlation
    (12 + 96 + 66 statistics per p): each within 5 sigma (sigma = 1 / sqrt(n); binomial for the rate)."""
    z = _stream_z(p, 1 << log2n)
    assert len(z) == 12 + 12 * len(LAGS) + 66
    worst = max(z, key=lambda k: abs(z[k]))
    print('p = %g, n = 2^%d: worst %s = %.2f sigma' % (p, log2n, worst, z[worst]))
    bad = {k: round(v, 2) for k, v in z.items() if not abs(v) <= 5.0}
    assert not bad, bad


def test_sites_of_a_step_do_not_share_a_mask():
    """The failure the parity tests cannot see: every site of a step drawing the same mask."""
    ks = [R.keep(4096, 0.1, SEED, off) for off in SITE_OFFSETS]
    for i in range(len(ks)):
        for j in range(i + 1, len(ks)):
            assert not np.array_equal(ks[i], ks[j])
