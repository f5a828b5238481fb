"""GPU: emo_favor_state_at, the FAVOR+ recurrent state of every row at its own length, against the float64 reference tests/favor_ref.py.  The
bound is the parent's own error: favor_attn_fwd(want_state=True) on the same k, v cut to the row's length, against the same float64, times 2
(the summation order differs: tiles of 32 tokens here, the forward's chunks and segments there).  Lengths one below, on and one above the
32-token tile edge, and a length of 1.  Tokens at and beyond a row's length must not reach its state, whatever they hold."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import favor_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
B, H, DH, NF, T = 3, 2, 64, 128, 96
_CASE = {}


def _inputs(dtype):
    """k, v as the kernel receives them ([B*T, H*dh] on the device, in `dtype`) and their float64 upcasts, omega; shared by the tests."""
    if dtype not in _CASE:
        gen = torch.Generator().manual_seed(11)
        k = torch.randn(B, T, H, DH, generator=gen) * 0.7
        v = torch.randn(B, T, H, DH, generator=gen)
        om = torch.randn(DH, NF // 2, generator=gen)
        dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
        kd, vd = k.to(dt), v.to(dt)
        _CASE[dtype] = (kd.reshape(B * T, H * DH).cuda().contiguous(), vd.reshape(B * T, H * DH).cuda().contiguous(), om.cuda().contiguous(),
                        kd.double(), vd.double(), om.double())
    return _CASE[dtype]


def _ref_state(k64, v64, om64, b, L):
    r = R.forward(k64[b:b + 1, :L], k64[b:b + 1, :L], v64[b:b + 1, :L], om64)
    return r['S'][0], r['z'][0]


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
@pytest.mark.parametrize('lens', [[1, 33, 96], [31, 32, 64]])
def test_state_at_matches_float64_within_twice_the_forwards_own_error(dtype, lens):
    from emo_disentanger_amd import ops
    kd, vd, omd, k64, v64, om64 = _inputs(dtype)
    S, z = ops.favor_state_at(kd, vd, omd, torch.tensor(lens, dtype=torch.int32, device='cuda'), B, T, H)
    torch.cuda.synchronize()
    S, z = S.cpu().double(), z.cpu().double()
    for b, L in enumerate(lens):
        Sr, zr = _ref_state(k64, v64, om64, b, L)
        # the parent's kernel on the row cut to its length: [1 * L, H * dh] views of the same device tensors
        kb, vb = kd.view(B, T, H * DH)[b, :L], vd.view(B, T, H * DH)[b, :L]
        _, _, Sp, zp = ops.favor_attn_fwd(kb, kb, vb, omd, 1, L, H, want_state=True)
        eS, ez = (Sp[0].cpu().double() - Sr).abs().max().item(), (zp[0].cpu().double() - zr).abs().max().item()
        gS, gz = (S[b] - Sr).abs().max().item(), (z[b] - zr).abs().max().item()
        print('state_error %s L=%d: S %.3e (forward %.3e), z %.3e (forward %.3e)' % (dtype, L, gS, eS, gz, ez))
        assert gS <= 2 * eS and gz <= 2 * ez, (dtype, b, L, gS, eS, gz, ez)


@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_tokens_beyond_a_rows_length_never_reach_its_state(dtype):
    from emo_disentanger_amd import ops
    kd, vd, omd = _inputs(dtype)[:3]
    for lens in ([1, 33, 96], [31, 32, 64]):
        ld = torch.tensor(lens, dtype=torch.int32, device='cuda')
        S0, z0 = ops.favor_state_at(kd, vd, omd, ld, B, T, H)
        kp, vp = kd.clone().view(B, T, H * DH), vd.clone().view(B, T, H * DH)
        for b, L in enumerate(lens):
            kp[b, L:] = 3.0e4                                  # large and finite in both dtypes
            vp[b, L:] = -1.0e30
        S1, z1 = ops.favor_state_at(kp.view(B * T, H * DH), vp.view(B * T, H * DH), omd, ld, B, T, H)
        torch.cuda.synchronize()
        assert torch.equal(S0, S1) and torch.equal(z0, z1), lens
        assert torch.isfinite(S1).all() and torch.isfinite(z1).all()


def test_state_at_refuses_what_it_cannot_run():
    from emo_disentanger_amd import _lib, ops
    kd, vd, omd = _inputs('fp32')[:3]
    ld = torch.tensor([1, 2, 3], dtype=torch.int32, device='cuda')
    with pytest.raises(AssertionError):
        ops.favor_state_at(kd, vd, omd, ld.long(), B, T, H)     # int64 lengths
    with pytest.raises(_lib.EmoError, match='unsupported'):
        ops.favor_state_at(kd[:, :96].contiguous(), vd[:, :96].contiguous(), omd[:48].contiguous(), ld, B, T, H)      # d_head 48
