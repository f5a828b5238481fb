"""TEST INFRASTRUCTURE: an EXACT reference for emo_gemm (include/emo_hip.h), on the host, with no tolerance to choose.

Operands are small integers: every entry is bf16-representable, every partial sum of a dot product and every intermediate of the epilogue
stays below 2^24 in magnitude, and every epilogue constant is a power of two (mul_scale = 2; p_drop = 0.5, whose keep multiplier is exactly
2).  Under those conditions every fp32 addition and every MFMA accumulation is exact WHATEVER the summation order, so the kernel family, the
ring geometry, the K-split count, atomics versus workspace and bias-first versus bias-last make no difference: an fp32 output must EQUAL the
integer result, a bf16 output must equal its one round-to-nearest-even conversion.  One dropped, duplicated or misplaced k-term, one stale
16-byte chunk, one edge row that reads its neighbour changes an integer by at least 1 and is seen at any K.

The epilogue follows the documented order:   +bias[n] -> (aux_out = value) -> ReLU -> *(mul_aux != 0) * mul_scale -> dropout -> +residual,
and `accumulate` adds the result onto the fp32 base.  The dropout keep decisions are tests/dropmask_ref.py (the host restatement of the device
stream, pinned to the device by tests/test_gpu_dropmask.py), element index m * N + n.

The product itself is a float64 BLAS matmul of integer-valued operands (|sum| < 2^53: exact), checked to be integral and held as int64 from
there on; tests/test_gemm_exact_ref_host.py pins it to NumPy's int64 matmul."""
import collections

import numpy as np
import torch

import dropmask_ref

LIMIT = 1 << 24          # |integer| < 2^24 is exactly representable in fp32, and so is every sum of such integers that stays below it

_mult_cache = {}

Expected = collections.namedtuple('Expected', 'out aux_out mask a_rowsum b_rowsum exact')


def ints(shape, lo, hi, seed, dtype=torch.bfloat16, zeros=0.0):
    """Integer-valued tensor uniform in [lo, hi] (inclusive) in `dtype`; zeros: share of entries forced to 0 (a multiplicative mask)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(lo, hi + 1, size=shape)
    if zeros:
        x = np.where(rng.random(size=shape) < zeros, 0, x)
    assert max(abs(lo), abs(hi)) <= 256, 'integers up to 256 are exact in bf16'
    return torch.from_numpy(x.astype(np.float32)).to(dtype)


def _i64(t, name):
    """int64 ndarray of an integer-valued tensor (any float dtype); raises when a value is not an integer."""
    d = t.detach().cpu().to(torch.float64).numpy()
    assert np.array_equal(d, np.rint(d)), '%s holds non-integers: the exact oracle does not apply' % name
    return d.astype(np.int64)


def product(A, B, a_trans, b_trans):
    """int64 [M, N] = op(A) @ op(B) for A stored [M, K] ([K, M] with a_trans) and B stored [N, K] ([K, N] with b_trans)."""
    a, b = _i64(A, 'A'), _i64(B, 'B')
    a = a.T if a_trans else a
    b = b if b_trans else b.T
    assert a.shape[1] == b.shape[0], (a.shape, b.shape)
    K = a.shape[1]
    amax, bmax = int(np.abs(a).max()), int(np.abs(b).max())
    assert amax * bmax * K < LIMIT, 'K = %d with |A| <= %d, |B| <= %d: a partial sum may reach 2^24, fp32 accumulation is no longer exact' % (K, amax, bmax)
    p = a.astype(np.float64) @ b.astype(np.float64)               # BLAS; |sum| < 2^24 << 2^53: exact in any order
    assert np.array_equal(p, np.rint(p))
    return p.astype(np.int64), amax * bmax * K


def to_dtype(exact, dtype):
    """The single conversion an exact integer result goes through: int64 -> fp32 (exact below 2^24) -> round-to-nearest-even to bf16."""
    assert int(np.abs(exact).max(initial=0)) < LIMIT
    t = torch.tensor(exact, dtype=torch.float32)
    return t if dtype == torch.float32 else t.to(dtype)


def pack_rows(mask):
    """bool [M, N] -> uint8 [M, N / 8], bit j of byte (m, n / 8) = column 8 (n / 8) + j: the row-major convention of ops.bitmask_rows."""
    m = np.asarray(mask, dtype=bool)
    assert m.shape[1] % 8 == 0
    return torch.from_numpy(np.packbits(m, axis=1, bitorder='little'))


def expected(A, B, *, a_trans=False, b_trans=False, bias=None, relu=False, want_aux=False, mul_aux=None, mul_scale=1.0, p_drop=0.0, seed=0, offset=0,
             residual=None, out_dtype=torch.float32, accumulate_base=None, want_mask=False, want_a_rowsum=None, want_b_rowsum=None):
    """Expected(out, aux_out, mask, a_rowsum, b_rowsum, exact) of one emo_gemm call.

    A, B: the operands AS STORED (host or device tensors, integer-valued).  bias [N]; mul_aux / residual [M, N] (EMO_MUL_NONZERO); relu: EMO_ACT_RELU;
    accumulate_base: the fp32 C the call accumulates onto (`accumulate=True`).  want_a_rowsum / want_b_rowsum: the vector the call adds its
    row sums to (a_rowsum[m] += sum_k op(A)[m][k], b_rowsum[n] += sum_k op(B)[n][k]).  out / aux_out come in out_dtype, mask is bool [M, N]
    (value after activation, mask multiply and dropout != 0), exact is the int64 result before the output conversion."""
    assert mul_scale in (1.0, 2.0, 4.0) and p_drop in (0.0, 0.5), 'epilogue constants must be powers of two (p_drop = 0.5: multiplier exactly 2)'
    v, bound = product(A, B, a_trans, b_trans)
    M, N = v.shape
    # the exactness condition, on the RANGES (not on the values this call happens to produce): every intermediate below 2^24
    if bias is not None:
        b = _i64(bias, 'bias')
        assert b.shape == (N,)
        bound += int(np.abs(b).max())
        v = v + b[None, :]
    aux = to_dtype(v, out_dtype) if want_aux else None
    if relu:
        v = np.maximum(v, 0)
    if mul_aux is not None:
        mz = _i64(mul_aux, 'mul_aux')
        assert mz.shape == (M, N)
        bound *= int(mul_scale)
        v = v * (mz != 0) * int(mul_scale)
    if p_drop:
        key = (M, N, p_drop, seed, offset)
        if key not in _mult_cache:                                   # (computed once per stream and shape, shared by the cases that draw it)
            _mult_cache.clear()
            _mult_cache[key] = dropmask_ref.multipliers((M, N), p_drop, seed, offset)
        mult = _mult_cache[key]
        assert set(np.unique(mult).tolist()) <= {0.0, 2.0}
        bound *= 2
        v = v * mult.astype(np.int64)
    mask = (v != 0) if want_mask else None
    if residual is not None:
        r = _i64(residual, 'residual')
        assert r.shape == (M, N)
        bound += int(np.abs(r).max())
        v = v + r
    if accumulate_base is not None:
        assert out_dtype == torch.float32
        c = _i64(accumulate_base, 'accumulate_base')
        assert c.shape == (M, N)
        bound += int(np.abs(c).max())
        v = v + c
    assert bound < LIMIT, 'the epilogue may reach %d >= 2^24: fp32 arithmetic is no longer exact' % bound
    rs_a = rs_b = None
    if want_a_rowsum is not None:
        a = _i64(A, 'A')
        s = (a.sum(0) if a_trans else a.sum(1)) + _i64(want_a_rowsum, 'a_rowsum')
        assert int(np.abs(a).sum(0 if a_trans else 1).max()) + int(np.abs(_i64(want_a_rowsum, 'a_rowsum')).max()) < LIMIT
        rs_a = torch.tensor(s, dtype=torch.float32)
    if want_b_rowsum is not None:
        b2 = _i64(B, 'B')
        s = (b2.sum(0) if b_trans else b2.sum(1)) + _i64(want_b_rowsum, 'b_rowsum')
        assert int(np.abs(b2).sum(0 if b_trans else 1).max()) + int(np.abs(_i64(want_b_rowsum, 'b_rowsum')).max()) < LIMIT
        rs_b = torch.tensor(s, dtype=torch.float32)
    return Expected(to_dtype(v, out_dtype), aux, mask, rs_a, rs_b, v)
