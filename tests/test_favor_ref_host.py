"""tests/favor_ref.py, the float64 reference behind tests/test_gpu_favor_edges.py, checked on the CPU:
  * it agrees with the oracle's three forms of causal_linear_attention, with float64 autograd through the quadratic form, and its predivided
    (dout_is_dn) variant agrees with the plain one;
  * a float32 evaluation of it (plain and chunked) stays inside the f32 bound, and a bf16-emulated chunked evaluation (omega, features, chunk
    matrices, carried state, dN, Jacobian operand and outputs rounded to bf16, float32 accumulation, the kernels' chunk sizes) inside the bf16
    bound, at every case of the GPU test's own lists;
  * every seeded defect, applied to the reference, breaks the bound (err / bound > 1) at a NAMED case of those lists, for the f32 and for the
    bf16 bounds — a bound or a case list too loose to see a defect fails here, not silently on the GPU."""
import pytest
import torch

import favor_ref as R
import test_gpu_favor_edges as G

NAMES = ('out', 'den', 'S', 'z', 'dq', 'dk', 'dv')


def _rand(B, T, H, dh, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, T, H, dh, generator=g, dtype=torch.float64) * s for s in (0.8, 0.8, 0.8, 1.0)]


@pytest.mark.parametrize('B,T,H,dh,nf,eps', [(2, 37, 3, 16, 32, 1e-6), (1, 70, 2, 32, 64, 0.25), (2, 20, 3, 64, 128, 0.0)])
def test_reference_agrees_with_the_oracle_and_with_autograd(B, T, H, dh, nf, eps):
    from oracle import model_ref
    q, k, v, dout = _rand(B, T, H, dh, 3)
    om = G.omega_of(dh, nf).double()
    f = R.forward(q, k, v, om, eps)
    for form, tol in (('quadratic', 1e-13), ('recurrent', 1e-13), ('prefix', 2e-6)):      # (the prefix form runs its causal product in float32 C)
        ref = model_ref.causal_linear_attention(q, k, v, om, eps=eps, form=form)
        assert float((f['out'] - ref).abs().max()) <= tol * float(ref.abs().max()), form
    Kf = model_ref.favor_features(k, om)
    assert torch.allclose(R.features(k, om), Kf, rtol=1e-13, atol=0)
    for got, ref in ((f['S'], torch.einsum('nlhf,nlhd->nhfd', Kf, v)), (f['z'], Kf.sum(1)),
                     (f['den'], torch.einsum('nlhf,nlhf->nhl', model_ref.favor_features(q, om), Kf.cumsum(1)) + eps)):
        assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    qa, ka, va = [t.clone().requires_grad_(True) for t in (q, k, v)]
    model_ref.causal_linear_attention(qa, ka, va, om, eps=eps, form='quadratic').backward(dout)
    b = R.backward(q, k, v, om, dout, eps)
    dn = R.backward(q, k, v, om, dout / f['den'].permute(0, 2, 1).unsqueeze(-1), eps, dn=True)
    for n, a in (('dq', qa), ('dk', ka), ('dv', va)):
        s = float(a.grad.abs().max())
        assert float((b[n] - a.grad).abs().max()) <= 1e-12 * s, n
        assert float((dn[n] - a.grad).abs().max()) <= 1e-12 * s, n + ' (predivided)'


def _evaluations(c, q, k, v, dout, om):
    """what must stay inside the bound of case c: (label, results)"""
    cs = G.chunks(c['fam'], c['dh'])
    if c['dn']:
        dout = G.dn_of(dout, R.forward(q, k, v, om.double(), c['eps'])['den']).double()
    if c['fam'] == 'f32':
        a = [t.float() for t in (q, k, v)]
        f = R.forward(*a, om, float(c['eps']))
        f.update({n: t for n, t in R.backward(*a, om, dout.float(), float(c['eps'])).items() if n in NAMES})
        return [('float32', f), ('float32 chunked', R.emulate(q, k, v, om, dout, c['eps'], cs, False))]
    return [('bf16 emulation', R.emulate(q, k, v, om, dout, c['eps'], cs, True, dn=c['dn']))]


def _bounds(c, ins):
    bd = G.inputs_and_bounds(c)[1]
    return G.bounds_of(c, *ins) if bd is None else bd


def _inside(c, loud=G.LOUD_SCALE):
    ins = G.make_inputs(c, loud=loud)
    bd = G.bounds_of(c, *ins) if loud != G.LOUD_SCALE else _bounds(c, ins)
    worst = 0.0
    for label, res in _evaluations(c, *ins):
        for n in NAMES:
            worst = max(worst, bd.ratio(n, res[n]))
    return worst


@pytest.mark.parametrize('group', ['a-f32', 'a-bf16', 'b', 'c', 'd', 'e'])
def test_reference_evaluations_stay_inside_their_own_bound(group):
    cases = {'b': G.CASES_B, 'c': G.CASES_C, 'd': G.CASES_D, 'e': G.CASES_E}.get(group)
    if cases is None:
        cases = [c for (fam, _, _), cs in G.CASES_A.items() if fam == group[2:] for c in cs]
    worst = {}
    for c in cases:
        r = _inside(c)
        worst[c['fam']] = max(worst.get(c['fam'], 0.0), r)
        assert r <= 1.0, '%s: err/bound = %.3f' % (G.key(c), r)
    print('worst err/bound of the reference evaluations:', worst)


def test_loud_scale_is_the_largest_that_stays_inside_the_bound():
    ok = [s for s in (2, 3, 4, 6) if all(_inside(c, loud=s) <= 1.0 for c in G.CASES_E)]
    assert ok and max(ok) == G.LOUD_SCALE
    for c in G.CASES_E:                                            # the first token's den does fall to eps
        f = R.forward(*G.make_inputs(c)[:3], G.omega_of(c['dh'], c['nf']).double(), c['eps'])
        assert float(f['den'][:, :, 0].max()) <= 1.5 * c['eps']


# ---------------------------------------------------------------------------------------------------- seeded defects
def _mutant(name, c, q, k, v, dout, om):
    """the reference with one defect, on case c: dict of the quantities it changes (None: the defect cannot show at this case)"""
    T, eps, dn = c['T'], c['eps'], c['dn']
    C = G.chunks(c['fam'], c['dh'])[0]
    if dn:
        dout = G.dn_of(dout, R.forward(q, k, v, om, eps)['den']).double()

    def both(qkvg=None, e=eps, **kw):
        a = (q, k, v, dout) if qkvg is None else qkvg
        f = R.forward(*a[:3], om, e, **{x: y for x, y in kw.items() if x in ('mask', 'ln_f')})
        f.update({n: t for n, t in R.backward(*a[:3], om, a[3], e, dn=dn, **kw).items() if n in NAMES})
        return f
    M = R.causal_mask(T)
    if name.startswith('mask_lt_'):
        Cm = int(name[8:])
        M[torch.arange(0, T, Cm), torch.arange(0, T, Cm)] = 0
        return both(mask=M)
    if name == 'chunk_state_dropped':
        if T <= C:
            return None
        M[C:, :C] = 0
        return both(mask=M)
    if name == 'segment_state_dropped':
        if c['segs'] == 1:
            return None
        Ts = G.seg_len(T, c['segs'])[1]
        M[Ts:, :Ts] = 0
        return both(mask=M)
    if name == 'tail_left_out_of_state':
        return None if T % C == 0 else {n: t for n, t in R.forward(q, k, v, om, eps, state_upto=T // C * C).items() if n in ('S', 'z')}
    if name == 'eps_left_out':
        return both(e=0.0)
    if name == 'eps_twice':
        return both(e=2 * eps)
    if name == 'dd_dropped':
        return both(no_dd=True)
    if name == 'dd_from_dout_in_dn_form':
        return both(dd_over_den=True) if dn else None
    if name == 'suma_dropped':
        return both(no_suma=True)
    if name == 'ln_f_left_out':
        return {n: t for n, t in R.forward(q, k, v, om, eps, ln_f=False).items() if n in ('den', 'S', 'z')}
    if name == 'stream_1_from_the_chunk_grid':
        if T % C == 0:
            return None
        B, _, H, dh = q.shape
        Tc = -(-T // C) * C

        def shift(t):
            flat = torch.cat([t.reshape(B * T, H, dh), torch.zeros(B * Tc, H, dh, dtype=t.dtype)])
            return torch.stack([flat[b * Tc:b * Tc + T] for b in range(B)])
        return both(qkvg=[shift(t) for t in (q, k, v, dout)])
    if name == 'head_mod_2':
        return both(qkvg=[torch.cat([t[:, :, :2], t[:, :, :1]], 2) for t in (q, k, v, dout)])
    raise KeyError(name)


def _c(fam, T, **kw):
    return G.case(fam, T, **kw)


# defect -> the case that catches it under the f32 bound, the case that catches it under the bf16 bound.  Where only one kind of case can show a
# defect it is said so: eps only where eps matters (0.25), the tail and the stream offset only where T is off the chunk grid, the segment state
# only in a segmented case, the predivided dD only in the dout_is_dn form (which exists for the bf16 slice kernels alone).
DEFECTS = {
    'mask_lt_16': (_c('f32', 17), _c('bf16', 17)),
    'mask_lt_32': (_c('f32', 33), _c('bf16', 33)),
    'mask_lt_64': (_c('f32', 65), _c('bf16', 65)),
    'chunk_state_dropped': (_c('f32', 33), _c('bf16', 65)),
    'segment_state_dropped': (_c('f32', 257, segs=2), _c('bf16', 257, segs=2)),
    'tail_left_out_of_state': (_c('f32', 33), _c('bf16', 65)),
    'eps_left_out': (_c('f32', 65, eps=0.25), _c('bf16', 65, eps=0.25)),                  # only the eps = 0.25 cases
    'eps_twice': (_c('f32', 65, eps=0.25), _c('bf16', 65, eps=0.25)),                     # only the eps = 0.25 cases
    'dd_dropped': (_c('f32', 17), _c('bf16', 15, dh=16, nf=32)),                              # bf16: the omega term of the bound hides it at d_head 64
    'dd_from_dout_in_dn_form': (None, _c('fs', 96, dn=True, cls='pos')),          # dout_is_dn only (bf16), and only where dD is a sum without cancellation (v, dout > 0)
    'suma_dropped': (_c('f32', 17), _c('bf16', 16, dh=16, nf=32)),                            # bf16: as dd_dropped
    'ln_f_left_out': (_c('f32', 1), _c('bf16', 1)),
    'stream_1_from_the_chunk_grid': (_c('f32', 17), _c('bf16', 17)),
    'head_mod_2': (_c('f32', 16), _c('bf16', 16)),
}


@pytest.mark.parametrize('name', list(DEFECTS))
def test_seeded_defect_breaks_the_bound_at_its_named_case(name):
    for c in DEFECTS[name]:
        if c is None:
            continue
        assert any(G.key(c) == G.key(x) for x in G.ALL_CASES), 'not a case of the GPU test: ' + G.key(c)
        ins = G.make_inputs(c)
        bd = _bounds(c, ins)
        m = _mutant(name, c, *ins[:4], ins[4].double())
        assert m is not None, G.key(c)
        r = max(bd.ratio(n, t) for n, t in m.items())
        print('%s at %s: err/bound = %.2f' % (name, G.key(c), r))
        assert r > 1.0, '%s is not caught at %s: err/bound = %.3f' % (name, G.key(c), r)
