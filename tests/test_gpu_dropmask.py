"""The library's dropout stream against tests/dropmask_ref.py, the NumPy restatement of the specification in csrc/emo_common.h — bit for bit.

Every other dropout-on test compares kernels with each other (a fused kernel against ops.dropout_apply of the plain result; the oracle parity
runs read their masks out of emo_dropout_apply).  Here the reference is outside the library: emo_dropout_apply itself, and one fused consumer
per indexing rule, are compared with the port directly.  The statistics of the stream are asserted on the port (tests/test_dropmask_host.py).

For the fused consumers the zero / non-zero pattern of the output is compared with the port's keep decisions.  An element whose value is exactly
zero BEFORE dropout says nothing and is excluded; each test counts those, asserts the count is at most 0.1 % and its inputs are chosen so that it
is 0 (sums of random normals; causal probabilities 1 / (i + 1))."""
import numpy as np
import pytest
import torch

import dropmask_ref as R

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
BIG = 4 * (4096 * 256 + 3)          # one quad more than 4096 blocks x 256 threads cover in one pass, plus two: the grid-stride loop runs twice
STREAMS = [(12345, 4105), ((0xDEADBEEF << 32) | 7, 3), (5, (0x1234567 << 32) | 4106), (2 ** 64 - 1, 2 ** 64 - 1)]


def _ops():
    from emo_disentanger_amd import ops
    return ops


def _r(*shape, seed=0, dt=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def _same_pattern(got, plain, keep_ref, what):
    """got != 0 exactly where the port keeps, on the elements whose undropped value `plain` is not exactly zero."""
    got, plain = got.detach().float().cpu().numpy().reshape(-1), plain.detach().float().cpu().numpy().reshape(-1)
    keep_ref = np.asarray(keep_ref).reshape(-1)
    excluded = plain == 0
    n_ex = int(excluded.sum())
    assert n_ex <= 1e-3 * plain.size, '%s: %d of %d elements are exactly zero before dropout' % (what, n_ex, plain.size)
    assert n_ex == 0, '%s: inputs were chosen to leave no exact zero, found %d' % (what, n_ex)
    bad = ((got != 0) != keep_ref) & ~excluded
    assert not bad.any(), '%s: %d of %d keep decisions differ from the port (first at linear index %d); excluded %d' % (
        what, int(bad.sum()), bad.size, int(np.argmax(bad)), n_ex)
    assert 0 < keep_ref.sum() < keep_ref.size


# ---------------------------------------------------------------------------------------------------- emo_dropout_apply
@pytest.mark.parametrize('p', [0.1, 0.25, 0.5])
@pytest.mark.parametrize('dt', DT)
def test_dropout_apply_of_ones_is_the_port(dt, p):
    ops = _ops()
    for n in (4, 1028, BIG):
        ones = torch.ones(n, device='cuda', dtype=dt)
        for seed, offset in (STREAMS if n != BIG else STREAMS[:2]):
            got = ops.dropout_apply(ones, p, seed, offset).float().cpu().numpy()
            ref = R.multipliers((n,), p, seed, offset)
            if dt == torch.bfloat16:
                ref = torch.from_numpy(ref).to(torch.bfloat16).float().numpy()          # the multiplier rounded once to the storage type
            else:
                assert set(np.unique(got).tolist()) <= {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}
            diff = got != ref
            assert not diff.any(), (n, seed, offset, int(diff.sum()), int(np.argmax(diff)))


def test_dropout_apply_p_zero_and_tiny_p():
    ops = _ops()
    x = _r(1028, seed=1).cuda()
    assert torch.equal(ops.dropout_apply(x, 0.0, 1, 2), x)
    p = 1.0 / 65536                                         # thr16 = 1: only the 16-bit field 0 is dropped
    ones = torch.ones(BIG, device='cuda')
    got = ops.dropout_apply(ones, p, 12345, 9).cpu().numpy()
    ref = R.multipliers((BIG,), p, 12345, 9)
    assert np.array_equal(got, ref) and 0 < int((ref == 0).sum()) < 200          # expected 64 of 4.2 M


# ---------------------------------------------------------------------------------------------------- fused consumers, one per indexing rule
@pytest.mark.parametrize('dt', DT)
def test_gemm_epilogue_unaligned_rows_draw_the_port_stream(dt):
    """N % 4 != 0: row m starts at linear index m N, not a multiple of 4 for odd m — the per-element path of drop_mult4 (index m N + n).
    bf16: operands and output are views into padded buffers (row pitches 40 / 40 / 56), the index stays m N + n of the LOGICAL shape."""
    ops = _ops()
    M, N, K = 70, 50, 37
    p, seed, offset = 0.25, (9 << 32) | 11, (1 << 32) | 3
    A, W = _r(M, K, seed=7, dt=dt), _r(N, K, seed=8, dt=dt, scale=0.3)
    if dt == torch.bfloat16:
        Ab, Wb = torch.zeros(72, 40, dtype=dt, device='cuda'), torch.zeros(56, 40, dtype=dt, device='cuda')
        Ab[:M, :K], Wb[:N, :K] = A.cuda(), W.cuda()
        Ag, Wg = Ab[:M, :K], Wb[:N, :K]
        new_out = lambda: torch.zeros(72, 56, dtype=dt, device='cuda')[:M, :N]
    else:
        Ag, Wg = A.cuda(), W.cuda()
        new_out = lambda: torch.zeros(M, N, dtype=dt, device='cuda')
    plain = ops.gemm(Ag, Wg, out=new_out())
    got = ops.gemm(Ag, Wg, out=new_out(), p_drop=p, seed=seed, offset=offset)      # (the library serves this shape: generic epilogue, per-element path)
    ref = A.double() @ W.double().T
    assert float((plain.double().cpu() - ref).abs().max()) <= (2e-5 if dt == torch.float32 else 3e-2) * float(ref.abs().max())
    keep = R.keep(M * N, p, seed, offset).reshape(M, N)
    _same_pattern(got, plain, keep, 'gemm %s' % dt)
    scale = float(R.make_drop(p, seed, offset)[3])
    k = torch.from_numpy(keep)
    err = (got.double().cpu() - plain.double().cpu() * scale)[k].abs()
    bound = plain.double().cpu().abs()[k] * scale * (2.0 ** -22 if dt == torch.float32 else 2.0 ** -7)
    assert bool((err <= bound).all())


@pytest.mark.parametrize('dt', DT)
def test_embed_fwd_draws_the_port_stream(dt):
    """index (b T + t) D + d"""
    ops = _ops()
    B, T, D, V = 3, 50, 68, 37
    p, seed, offset = 0.1, 12345, (2 << 32) | 4096
    E, pe = _r(V, D, seed=1), _r(T + 5, D, seed=2)
    tok = torch.randint(0, V, (B, T), generator=torch.Generator().manual_seed(0))
    plain = ops.embed_fwd(tok.cuda(), None, E.cuda(), None, pe.cuda(), dt, 8.0, pos0=5)
    got = ops.embed_fwd(tok.cuda(), None, E.cuda(), None, pe.cuda(), dt, 8.0, pos0=5, p_drop=p, seed=seed, offset=offset)
    _same_pattern(got, plain, R.keep(B * T * D, p, seed, offset), 'embed_fwd %s' % dt)


@pytest.mark.parametrize('dt, M, D', [(torch.float32, 37, 64), (torch.bfloat16, 37, 64), (torch.bfloat16, 37, 512)])
def test_layernorm_bwd_dx_drop_draws_the_port_stream(dt, M, D):
    """index row D + c; bf16 at D = 512 is the 16-byte kernel (two aligned quads per lane), the others the generic one."""
    ops = _ops()
    p, seed, offset = 0.5, (3 << 32) | 9, 4107
    x, dy, dres = _r(M, D, seed=1, dt=dt).cuda(), _r(M, D, seed=4, dt=dt).cuda(), _r(M, D, seed=5, dt=dt).cuda()
    gm, bt = (_r(D, seed=2) * 0.1 + 1).cuda(), _r(D, seed=3).cuda()
    _, mean, rstd = ops.layernorm_fwd(x, gm, bt)
    dg, db, dcol = torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')
    dx, dxd = ops.layernorm_bwd(dy, x, gm, mean, rstd, dg, db, dres=dres, want_drop=True, p_drop=p, seed=seed, offset=offset, dcol=dcol)
    _same_pattern(dxd, dx, R.keep(M * D, p, seed, offset), 'layernorm_bwd %s D=%d' % (dt, D))
    mult = torch.from_numpy(R.multipliers((M, D), p, seed, offset))
    assert torch.equal(dxd.float().cpu(), (dx.float().cpu() * mult).to(dt).float())          # 1 / (1 - 0.5) = 2: exact in both types


@pytest.mark.parametrize('dt', DT)
def test_softmax_attention_probabilities_draw_the_port_stream(dt):
    """index ((b H + h) T + i) T + j, read out of the forward kernel with q = k = 0 and V = identity (every causal probability is 1 / (i + 1) > 0)."""
    from test_gpu_dropout_parity import attention_keep_from_kernel
    B, T, H, dh = 1, 64, 2, 64
    p, seed, offset = 0.1, 12345, 4096 + 8 + 1
    keep = attention_keep_from_kernel(B, T, H, dh, p, seed, offset, dt).numpy()
    ref = R.keep(B * H * T * T, p, seed, offset).reshape(B, H, T, T)
    causal = np.tril(np.ones((T, T), dtype=bool))[None, None]
    excluded = 0                                            # 1 / (i + 1) is never zero
    bad = (keep != ref) & causal
    assert not bad.any(), '%d of %d causal keep decisions differ from the port; excluded %d' % (int(bad.sum()), int(causal.sum()) * B * H, excluded)
    assert 0 < ref[np.broadcast_to(causal, ref.shape)].sum() < causal.sum() * B * H
