"""The exact GEMM oracle (tests/gemm_exact_ref.py) checked on the host, without a GPU: against NumPy's int64 matmul and an independently written
float64 epilogue on random shapes, its exactness guard, and its mask packing against ops.bitmask_rows' layout convention."""
import numpy as np
import pytest
import torch

import dropmask_ref
import gemm_exact_ref as X


def _rand_case(rng):
    M, N, K = int(rng.integers(1, 70)), int(rng.integers(1, 70)), int(rng.integers(1, 300))
    a_trans, b_trans = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    A = X.ints((K, M) if a_trans else (M, K), -3, 3, int(rng.integers(1 << 30)))
    B = X.ints((K, N) if b_trans else (N, K), -3, 3, int(rng.integers(1 << 30)))
    return M, N, K, a_trans, b_trans, A, B


def test_product_is_the_int64_product_and_the_fp32_product():
    rng = np.random.default_rng(1)
    for _ in range(20):
        M, N, K, at, bt, A, B = _rand_case(rng)
        a = A.double().numpy().astype(np.int64)
        b = B.double().numpy().astype(np.int64)
        want = (a.T if at else a) @ (b if bt else b.T)               # NumPy's integer matmul: no floating point anywhere
        got = X.expected(A, B, a_trans=at, b_trans=bt)
        assert np.array_equal(got.exact, want)
        assert got.out.dtype == torch.float32 and np.array_equal(got.out.numpy().astype(np.int64), want)
        # the premise of the whole oracle, on this CPU: an fp32 product of these operands is the integer product
        f32 = (A.float().T if at else A.float()) @ (B.float() if bt else B.float().T)
        assert torch.equal(f32, got.out)


@pytest.mark.parametrize('out_dtype', [torch.float32, torch.bfloat16])
def test_epilogue_matches_a_float64_epilogue_in_the_documented_order(out_dtype):
    rng = np.random.default_rng(2)
    for it in range(24):
        M, N, K, at, bt, A, B = _rand_case(rng)
        if it % 3 == 0:
            A = A + 3                                                # the shifted range [0, 6]: large outputs at a small K
        bias = X.ints((N,), -8, 8, it, torch.float32) if it & 1 else None
        res = X.ints((M, N), -64, 64, it + 100, out_dtype) if it & 2 else None
        mul = X.ints((M, N), -64, 64, it + 200, out_dtype, zeros=0.4) if it & 4 else None
        base = X.ints((M, N), -64, 64, it + 300, torch.float32) if (it & 8 and out_dtype == torch.float32) else None
        relu, p = bool(it & 16) or it % 5 == 0, 0.5 if it % 2 == 0 else 0.0
        got = X.expected(A, B, a_trans=at, b_trans=bt, bias=bias, relu=relu, want_aux=True, mul_aux=mul, mul_scale=2.0, p_drop=p, seed=7, offset=it,
                         residual=res, out_dtype=out_dtype, accumulate_base=base, want_mask=True)
        z = (A.double().T if at else A.double()) @ (B.double() if bt else B.double().T)
        if bias is not None:
            z = z + bias.double()
        assert torch.equal(got.aux_out, z.float().to(out_dtype))
        if relu:
            z = z.clamp_min(0)
        if mul is not None:
            z = z * (mul.double() != 0) * 2.0
        if p:
            z = z * torch.from_numpy(dropmask_ref.multipliers((M, N), p, 7, it)).double()
        assert torch.equal(torch.from_numpy(got.mask), z != 0)
        if res is not None:
            z = z + res.double()
        if base is not None:
            z = z + base.double()
        assert torch.equal(got.out, z.float().to(out_dtype)) and got.out.dtype == out_dtype
        assert np.array_equal(got.exact, z.numpy().astype(np.int64))


def test_row_sums_follow_the_stored_layouts():
    A, B = X.ints((96, 20), -3, 3, 1), X.ints((96, 24), -3, 3, 2)     # the weight-gradient layout: A stored [K, M], B stored [K, N]
    a0, b0 = X.ints((20,), -64, 64, 3, torch.float32), X.ints((24,), -64, 64, 4, torch.float32)
    got = X.expected(A, B, a_trans=True, b_trans=True, want_a_rowsum=a0, want_b_rowsum=b0)
    assert torch.equal(got.a_rowsum, a0 + A.float().sum(0)) and torch.equal(got.b_rowsum, b0 + B.float().sum(0))


def test_bf16_rounding_is_not_trivial_where_the_tests_need_it():
    # a bf16 accumulator or a double rounding shows only on outputs above 256: K = 512 in [-3, 3] has some, the shifted range has many at K = 32
    A, B = X.ints((256, 512), -3, 3, 1), X.ints((256, 512), -3, 3, 2)
    got = X.expected(A, B, out_dtype=torch.bfloat16)
    assert int(np.abs(got.exact).max()) > 256 and not np.array_equal(got.out.double().numpy().astype(np.int64), got.exact)
    got = X.expected(X.ints((64, 32), 0, 6, 3), X.ints((64, 32), -3, 3, 4) + 3, out_dtype=torch.bfloat16)
    assert float((np.abs(got.exact) > 256).mean()) > 0.3


def test_exactness_guard_raises():
    A, B = X.ints((8, 64), -3, 3, 1), X.ints((8, 64), -3, 3, 2)
    with pytest.raises(AssertionError, match='2\\^24'):               # a product whose range could reach 2^24: K * |a| * |b|
        X.expected(A * 64, B * 64 * 16)
    with pytest.raises(AssertionError, match='2\\^24'):               # the range, not the values: 2^23 of product range doubled by the mask scale
        X.expected(torch.full((8, 1 << 15), 16.0), torch.full((8, 1 << 15), 16.0).clone(), mul_aux=torch.ones(8, 8), mul_scale=2.0)
    with pytest.raises(AssertionError, match='powers of two'):
        X.expected(A, B, p_drop=0.1)
    with pytest.raises(AssertionError, match='non-integers'):
        X.expected(A * 0.5, B)
    X.expected(A, B, mul_aux=torch.ones(8, 8), mul_scale=2.0, p_drop=0.5)   # (the same request inside the range passes)


def test_mask_bits_follow_the_row_major_convention_of_bitmask_rows():
    """A synthetic mask written byte by byte in the TILED layout emo_hip.h documents for mask_out, unpacked by ops.bitmask_rows, equals
    pack_rows of the same mask: byte (m, n / 8), bit j = column 8 (n / 8) + j."""
    from emo_disentanger_amd import ops
    M, N = 64, 128
    rng = np.random.default_rng(5)
    mask = rng.random((M, N)) < 0.4
    tiled = np.zeros(M * N // 8, dtype=np.uint8)
    for m in range(M):
        for n8 in range(N // 8):
            n = 8 * n8
            byte = ((m // 32) * (N // 64) + n // 64) * 256 + ((n % 32) // 8 * 16 + m % 16) * 4 + (m % 32) // 16 * 2 + (n % 64) // 32
            tiled[byte] = sum(int(mask[m, n + j]) << j for j in range(8))
    rows = ops.bitmask_rows(torch.from_numpy(tiled), M, N)
    assert torch.equal(rows, X.pack_rows(mask))
    bits = (rows[:, :, None] >> torch.arange(8, dtype=torch.uint8)) & 1
    assert np.array_equal(bits.reshape(M, N).bool().numpy(), mask)
