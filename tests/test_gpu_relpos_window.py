"""GPU: the sliding-window (banded) forward of the stage-1 relative-position attention, emo_attn [relpos, fwd] with window = W > 0, alone:
score[i][j] for max(0, i - W) <= j <= i, against a float64 NumPy banded attention written here, against the unwindowed kernel where the band
holds every key, and against the one-token decode kernel whose window it restates."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
B, H, DH = 2, 2, 64
HD = H * DH
# Copied by value from tests/test_gpu_kernels.py: _tol (2e-5 fp32 / 3e-2 bf16, relative to the reference's scale) and the factors that
# test_relpos_attention_fwd_and_decode applies to the unwindowed forward: mult=3 on out (and on the decode result, against the same
# reference), mult=10 at the fp32 tolerance and scale 1.0 on zden.  lse, which that test does not look at, takes out's constants.
TOL = {torch.float32: 2e-5, torch.bfloat16: 3e-2}
OUT_MULT, ZDEN_MULT = 3, 10


def _r(*shape, seed=0, dt=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt)


_INPUTS = {}


def _inputs(T, dt):
    """qkv [B*T, 3*HD], R [T, HD] in the compute dtype (so the reference sees the rounded values), u, vb [H, dh] fp32; made once per (T, dtype)."""
    if (T, dt) not in _INPUTS:
        _INPUTS[(T, dt)] = (_r(B * T, 3 * HD, seed=1, dt=dt, scale=0.7), _r(T, HD, seed=2, dt=dt, scale=0.7), _r(H, DH, seed=3, scale=0.3),
                            _r(H, DH, seed=4, scale=0.3))
    return _INPUTS[(T, dt)]


_REFS = {}


def _band_ref(T, dt, W):
    """float64: out [B, T, H, dh], lse [B, H, T], zden [B, H, T] of the banded attention (W = None: causal), the kernel's definitions:
    lse = log sum_j exp(score), out = softmax v / (1 + 1e-8), zden = 1 + 1e-8 (no dropout)."""
    if (T, dt, W) not in _REFS:
        qkv, R, u, vb = (t.double().numpy() for t in _inputs(T, dt))
        q, k, v = (qkv[:, i * HD:(i + 1) * HD].reshape(B, T, H, DH) for i in range(3))
        Rh = R.reshape(T, H, DH)
        i, j = np.arange(T)[:, None], np.arange(T)[None, :]
        AC = np.einsum('bihd,bjhd->bhij', q + u, k)
        BD = np.einsum('bihd,ijhd->bhij', q + vb, Rh[np.clip(i - j, 0, T - 1)])
        sc = (AC + BD) / DH ** 0.5
        keep = (j <= i) if W is None else ((j <= i) & (j >= i - W))
        sc = np.where(keep, sc, -np.inf)
        m = sc.max(-1, keepdims=True)
        e = np.exp(sc - m)
        l = e.sum(-1, keepdims=True)
        p = e / l
        out = np.einsum('bhij,bjhd->bihd', p / (p.sum(-1, keepdims=True) + 1e-8), v)
        _REFS[(T, dt, W)] = (out, (m + np.log(l))[..., 0], np.full((B, H, T), 1.0 + 1e-8))
    return _REFS[(T, dt, W)]


def _fwd(T, dt, window, n_dist=None):
    from emo_disentanger_amd import ops
    qkv, R, u, vb = _inputs(T, dt)
    qc = qkv.cuda()
    Rc = R.cuda() if n_dist is None else R[:n_dist].contiguous().cuda()
    return ops.relpos_attn_fwd(qc[:, :HD], qc[:, HD:2 * HD], qc[:, 2 * HD:], Rc, u.cuda(), vb.cuda(), B, T, H, window=window)


def _err(got, ref):
    return float(np.abs(got.detach().double().cpu().numpy() - ref).max())


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('T', [130, 200])
@pytest.mark.parametrize('W', [1, 63, 64, 65, 100])
def test_band_edges_against_float64(dt, T, W):
    # W = 63 / 64 / 65: the edge inside a tile, on a tile boundary, across two tiles; W = 1 at T = 200: most key tiles are skipped
    ref_out, ref_lse, ref_zden = _band_ref(T, dt, W)
    out, lse, zden = _fwd(T, dt, W)
    e_out, e_lse, e_zden = _err(out.view(B, T, H, DH), ref_out), _err(lse, ref_lse), _err(zden, ref_zden)
    s_out, s_lse = float(np.abs(ref_out).max()), float(np.abs(ref_lse).max())
    print('T %d W %d %s: out %.3e (scale %.3e)  lse %.3e (scale %.3e)  zden %.3e' % (T, W, dt, e_out, s_out, e_lse, s_lse, e_zden))
    assert e_out <= OUT_MULT * TOL[dt] * s_out
    assert e_lse <= OUT_MULT * TOL[dt] * s_lse
    assert e_zden <= ZDEN_MULT * TOL[torch.float32] * 1.0


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('T', [130, 200])
def test_a_band_that_holds_every_key_is_bit_identical_to_no_window(dt, T):
    base = _fwd(T, dt, 0)
    for W in (T - 1, T, T + 70):
        for a, b in zip(_fwd(T, dt, W), base):
            assert torch.equal(a, b), W


@pytest.mark.parametrize('dt', DT)
def test_windowed_forward_agrees_with_the_decode_kernel_row_by_row(dt):
    from emo_disentanger_amd import ops
    T, W = 130, 64
    qkv, R, u, vb = _inputs(T, dt)
    out, _, _ = _fwd(T, dt, W)
    x3 = qkv.cuda().view(B, T, 3 * HD)
    Rc, uc, vc_ = R.cuda(), u.cuda(), vb.cuda()
    kc, vc = torch.zeros(B, T, HD, dtype=dt, device='cuda'), torch.zeros(B, T, HD, dtype=dt, device='cuda')
    lens = torch.zeros(B, dtype=torch.long, device='cuda')
    rows = []
    for i in range(T):
        lens += 1
        row = x3[:, i].contiguous()
        rows.append(ops.relpos_attn_decode(row[:, :HD], kc, vc, lens, H, Rc, uc, vc_, mem_len=W, k_new=row[:, HD:2 * HD], v_new=row[:, 2 * HD:]))
    dec = torch.stack(rows, 1).double().cpu().numpy()                      # [B, T, HD]
    ref_out = _band_ref(T, dt, W)[0]
    err = np.abs(out.view(B, T, HD).double().cpu().numpy() - dec).reshape(B, T, -1).max((0, 2))
    print('forward vs decode, %s: max %.3e at row %d (scale %.3e)' % (dt, err.max(), int(err.argmax()), np.abs(ref_out).max()))
    # the existing test holds both kernels to the same reference at OUT_MULT * tol * scale; that bound between the two of them, row by row
    assert (err <= OUT_MULT * TOL[dt] * float(np.abs(ref_out).max())).all()


def _library_message(excinfo):
    """The library's own text: check() puts 'libemo_hip error <rc>: ' in front of it."""
    text = str(excinfo.value)
    assert text.startswith('libemo_hip error -1: ')                       # -1: refused on the host, nothing was launched
    return text[len('libemo_hip error -1: '):]


def test_window_is_refused_outside_the_relpos_forward():
    from emo_disentanger_amd import ops
    from emo_disentanger_amd._lib import EmoError
    T, dt = 130, torch.float32
    qkv, R, u, vb = _inputs(T, dt)
    qc, Rc, uc, vc = qkv.cuda(), R.cuda(), u.cuda(), vb.cuda()
    q, k, v = qc[:, :HD], qc[:, HD:2 * HD], qc[:, 2 * HD:]
    out, dout, dq, dq_rel = (torch.zeros(B * T, HD, device='cuda') for _ in range(4))
    lse, zden = torch.zeros(B, H, T, device='cuda'), torch.ones(B, H, T, device='cuda')
    with pytest.raises(EmoError) as e:                                     # the query-tile backward pass
        ops._attn(ops.ATTN_RELPOS, ops.ATTN_BWD, q, k, v, B, T, H, r_dist=ops.ptr(Rc), ld_r=HD, n_dist=T, r_w_bias=ops.ptr(uc), r_r_bias=ops.ptr(vc),
                  out=ops.ptr(out), dout=ops.ptr(dout), ld_out=HD, lse=ops.ptr(lse), zden=ops.ptr(zden), dq=ops.ptr(dq), dq_rel=ops.ptr(dq_rel),
                  ld_d=HD, ld_rel=HD, window=64)
    assert _library_message(e).startswith('emo_attn[relpos, bwd]: ') and 'window' in _library_message(e)
    with pytest.raises(EmoError) as e:                                     # another kind
        ops._attn(ops.ATTN_SOFTMAX, ops.ATTN_FWD, q, k, v, B, T, H, out=ops.ptr(out), ld_out=HD, lse=ops.ptr(lse), window=64)
    assert _library_message(e).startswith('emo_attn[softmax, fwd]: ') and 'window' in _library_message(e)
    with pytest.raises(EmoError) as e:                                     # with dropout
        ops.relpos_attn_fwd(q, k, v, Rc, uc, vc, B, T, H, p_drop=0.1, seed=1, window=64)
    assert _library_message(e).startswith('emo_attn[relpos, fwd]: ') and 'p_drop' in _library_message(e)
    R64 = Rc[:64].contiguous()
    with pytest.raises(EmoError) as e:                                     # fewer rows than the band reaches
        ops.relpos_attn_fwd(q, k, v, R64, uc, vc, B, T, H, window=64)
    assert _library_message(e).startswith('emo_attn[relpos, fwd]: ') and 'a row for every distance' in _library_message(e)


@pytest.mark.parametrize('dt', DT)
@pytest.mark.parametrize('T,W', [(130, 64), (200, 1), (200, 100)])
def test_a_distance_table_of_window_plus_one_rows_is_enough(dt, T, W):
    full = _fwd(T, dt, W)
    small = _fwd(T, dt, W, n_dist=W + 1)
    for a, b in zip(small, full):
        assert torch.equal(a, b)
