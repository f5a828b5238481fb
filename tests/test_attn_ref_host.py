"""tests/attn_ref.py checked on the host, without the kernels: the float64 references against torch's own attention and against the reference
model's pad-and-view relative shift, and the condition every EXACT assertion of tests/test_gpu_attn_train_edges.py rests on — the selector
inputs give probabilities that are exactly one-hot once rounded to fp32, for every (T, d_head, map or distance, window) the GPU file runs."""
import math

import numpy as np
import pytest
import torch

import attn_ref as ar

F64 = torch.float64


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=F64) * scale


@pytest.mark.parametrize('B,T,H,dh', [(2, 1, 3, 16), (2, 17, 3, 32), (1, 65, 3, 64), (2, 129, 2, 64)])
def test_softmax_ref_equals_torch_sdpa(B, T, H, dh):
    q, k, v = [_r(B, T, H, dh, seed=s) for s in (1, 2, 3)]
    out, lse = ar.softmax_ref(q, k, v)
    ref = torch.nn.functional.scaled_dot_product_attention(ar._bh(q), ar._bh(k), ar._bh(v), is_causal=True)
    assert float((out - ar._bh(ref)).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))
    s = (ar._bh(q) @ ar._bh(k).transpose(-1, -2)) / math.sqrt(dh)
    for i in (0, T - 1):                                           # lse of a row = log of the plain sum over the keys it sees
        assert torch.allclose(lse[:, :, i], torch.log(torch.exp(s[:, :, i, :i + 1]).sum(-1)), rtol=0, atol=1e-12)
    # a mask multiplies the probabilities after the softmax (HF GPT2Attention._attn: softmax -> attn_dropout -> @ v)
    m = (torch.rand(B, H, T, T, generator=torch.Generator().manual_seed(4), dtype=F64) > 0.25).double() / 0.75
    out_m, lse_m = ar.softmax_ref(q, k, v, m)
    p = torch.softmax(s.masked_fill(torch.triu(torch.ones(T, T), 1).bool(), -float('inf')), -1)
    assert torch.allclose(out_m, ar._bh((p * m) @ ar._bh(v)), rtol=0, atol=1e-13) and torch.equal(lse, lse_m)


@pytest.mark.parametrize('B,T,H,dh', [(2, 1, 3, 16), (2, 17, 3, 32), (1, 65, 3, 64), (2, 130, 2, 16)])
def test_relpos_ref_equals_the_pad_and_view_shift(B, T, H, dh):
    """_relattn_ref's formula (tests/test_gpu_kernels.py) with BD formed as the reference model does: dense (q + vb).R^T over the position rows
    (row p = distance T - 1 - p), re-labelled by rel_shift, time-major [i, j, b, h]."""
    from oracle.txl_ref import rel_shift
    q, k, v = [_r(B, T, H, dh, seed=s, scale=0.7) for s in (1, 2, 3)]
    R, u, vb = _r(T + 3, H, dh, seed=4, scale=0.7), _r(H, dh, seed=5, scale=0.3), _r(H, dh, seed=6, scale=0.3)
    ac = torch.einsum('ibhd,jbhd->ijbh', (q + u).transpose(0, 1), k.transpose(0, 1))
    r_pos = R[:T].flip(0)                                          # the reference's r_head_k: row p holds distance T - 1 - p
    bd = rel_shift(torch.einsum('ibhd,phd->ipbh', (q + vb).transpose(0, 1), r_pos))
    s = (ac + bd) / dh ** 0.5
    s = s.masked_fill(torch.triu(torch.ones(T, T), 1).bool()[:, :, None, None], -float('inf'))
    p = torch.softmax(s, 1)
    p = p / (p.sum(1, keepdim=True) + 1e-8)
    ref = torch.einsum('ijbh,jbhd->bihd', p, v.transpose(0, 1))
    out, lse, zden = ar.relpos_ref(q, k, v, R, u, vb)
    assert float((out - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))
    assert torch.allclose(lse, torch.logsumexp(s, 1).permute(1, 2, 0), rtol=0, atol=1e-12)
    assert torch.allclose(zden, torch.full_like(zden, 1.0 + 1e-8), rtol=0, atol=1e-14)
    # a window W keeps the keys i - W .. i: the full rows restricted to the band and renormalised
    W = 5
    out_w, _, _ = ar.relpos_ref(q, k, v, R, u, vb, window=W)
    band = (torch.arange(T)[:, None] - torch.arange(T)[None, :] <= W)[:, :, None, None]
    pw = torch.softmax(s.masked_fill(~band, -float('inf')), 1)
    pw = pw / (pw.sum(1, keepdim=True) + 1e-8)
    assert torch.allclose(out_w, torch.einsum('ijbh,jbhd->bihd', pw, v.transpose(0, 1)), rtol=0, atol=1e-12)
    # dropout: softmax -> mask -> p / (sum p + 1e-8); zden is that sum
    m = (torch.rand(B, H, T, T, generator=torch.Generator().manual_seed(7), dtype=F64) > 0.25).double() / 0.75
    out_m, lse_m, zden_m = ar.relpos_ref(q, k, v, R, u, vb, mask=m)
    pm = torch.softmax(s, 1) * m.permute(2, 3, 0, 1)
    assert torch.allclose(zden_m, pm.sum(1).permute(1, 2, 0) + 1e-8, rtol=0, atol=1e-14) and torch.equal(lse_m, lse)
    assert torch.allclose(out_m, torch.einsum('ijbh,jbhd->bihd', pm / (pm.sum(1, keepdim=True) + 1e-8), v.transpose(0, 1)), rtol=0, atol=1e-12)


def _exact_in(x, dt):
    return torch.equal(x.to(dt).double(), x)


@pytest.mark.parametrize('T,dh', ar.SEL_GENERIC + ar.SEL_FUSED32)
@pytest.mark.parametrize('names', ar.SEL_MAPS)
def test_softmax_selector_probabilities_are_one_hot_in_fp32(T, dh, names):
    B, H = 2, 3
    maps = ar.selector_maps(T)
    pis = [maps[n] for n in names]
    for pi in pis:
        assert bool((pi <= torch.arange(T)).all()) and bool((pi >= 0).all())
    q, k, v = ar.softmax_selector(B, T, H, dh, pis, seed=T + dh)
    assert all(_exact_in(x, torch.bfloat16) for x in (q, k, v))
    for b in range(B):
        for h in range(H):
            assert len(torch.unique(v[b, :, h], dim=0)) == T       # distinct rows: a wrong key cannot hide behind an equal row
    assert not torch.equal(v[0], v[1])
    p, lse = ar.softmax_probs(q, k)
    assert ar.one_hot_f32(p, torch.stack(pis))
    out, _ = ar.softmax_ref(q, k, v)
    for h, pi in enumerate(pis):
        assert torch.equal(out[:, :, h].float(), v[:, pi, h].float())
        assert torch.allclose(lse[:, h], torch.full((B, T), ar.G * dh / math.sqrt(dh), dtype=F64), rtol=1e-15, atol=0)
    # the gap to the second-best key is at least 2 G / sqrt(dh): exp of it is 0 in fp32, base e and base 2
    s = (ar._bh(q) @ ar._bh(k).transpose(-1, -2)) / math.sqrt(dh)
    s = s.masked_fill(ar._dead(T), -float('inf'))
    top = torch.topk(s[:, :, 1:], 2, -1).values if T > 1 else None
    if top is not None:
        gap = float((top[..., 0] - top[..., 1]).min())
        assert gap >= 2 * ar.G / math.sqrt(dh) - 1e-9 and np.exp(np.float32(-gap)) == 0.0
    # gradients of the float64 reference for integer dout: dv = the integer sums, dq = dk = 0 once rounded to fp32
    dout = ar.small_int_dout(B, T, H, dh, seed=T)
    ql, kl, vl = [x.clone().requires_grad_(True) for x in (q, k, v)]
    ar.softmax_ref(ql, kl, vl)[0].backward(dout)
    assert torch.equal(vl.grad.float(), ar.softmax_selector_dv(dout, pis).float())
    assert not ql.grad.float().any() and not kl.grad.float().any()
    # every integer sum the kernels form stays below 2^24 (exact in fp32 whatever the order): dout.v, and the sums of dout rows (|dv| <= 3 T:
    # the fp32 accumulator is exact and a bf16 dv is ITS one rounding, which is what the GPU file compares with)
    assert float(dout.abs().amax()) * float(v.abs().amax()) * dh < 2 ** 24 and 3 * T < 2 ** 24


@pytest.mark.parametrize('dh', [16, 32, 64])
def test_bf16_backward_recomputes_a_selected_probability_that_rounds_to_one(dh):
    """The bf16 backward kernels recompute p = exp2(s c2 - lse log2e) from the STORED lse: the exponent is a difference of two rounded numbers of
    magnitude G sqrt(dh) log2e, not an exact 0.  dv is still the exact integer sum because p reaches the MFMA as a bf16 value: it must round to 1."""
    for fused in ((False, True) if dh == 64 else (False,)):
        p = ar.bf16_backward_probability(ar.G * dh, dh, fused)
        print('[attn_ref_host] d_head %d%s: recomputed p = %.7f' % (dh, ' (32 x 32)' if fused else '', float(p)))
        assert float(torch.tensor(float(p)).bfloat16()) == 1.0


@pytest.mark.parametrize('T', ar.SEL_RELPOS_T)
def test_relpos_selector_probabilities_are_one_hot_in_fp32(T):
    B, H, dh = 2, 3, ar.SEL_RELPOS_DH
    assert np.exp(np.float32(-ar.G / math.sqrt(dh))) == 0.0 and np.exp2(np.float32(-ar.G / math.sqrt(dh) * 1.4426950408889634)) == 0.0
    assert np.float32(1.0) + np.float32(1e-8) == np.float32(1.0)           # zden of a selected row as fp32 stores it
    for dstar in ar.relpos_dstar(T):
        q, k, v, R, u, vb = ar.relpos_selector(B, T, H, dh, dstar, seed=T)
        assert all(_exact_in(x, torch.bfloat16) for x in (q, k, v, R)) and _exact_in(vb, torch.float32)
        for w in ar.relpos_windows(dstar):
            sel = ar.relpos_selected(T, dstar, w)
            a, lse, zden = ar.relpos_probs(q, k, R, u, vb, window=w)
            assert ar.one_hot_f32(a, sel), (dstar, w)
            out = ar.relpos_ref(q, k, v, R, u, vb, window=w)[0]
            i = torch.arange(T)
            for h in range(H):
                rows = torch.nonzero(sel[h] >= 0)[:, 0]
                assert torch.equal(out[:, rows, h].float(), v[:, sel[h, rows], h].float())
                assert torch.equal(zden[:, h, rows].float(), torch.ones(B, len(rows)))
                # every other row is uniform over the keys it sees
                rest = torch.nonzero(sel[h] < 0)[:, 0]
                n_seen = (i[rest] + 1) if w <= 0 else torch.minimum(i[rest] + 1, torch.tensor(w + 1))
                want = (~ar._dead(T, w))[rest].double() / n_seen[:, None].double() / (1.0 + 1e-8)
                assert torch.allclose(a[:, h, rest], want[None].expand(B, -1, -1), rtol=0, atol=1e-15)
        # every selected distance is hit by some row, and with window = d* - 1 by none
        for h, d in enumerate(dstar):
            assert int((ar.relpos_selected(T, dstar, 0)[h] >= 0).sum()) == T - d
            if d >= 2:
                assert int((ar.relpos_selected(T, dstar, d - 1)[h] >= 0).sum()) == 0
