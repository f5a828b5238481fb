"""The training passes of the SOFTMAX and RELPOS kinds of emo_attn (GPU) at the edges of their tiles: the generic kernels of
csrc/emo_softmax_attn.hip (64-row query tiles, 16 rows per wave, the causal mask on the diagonal tile, the relative skew c = t - j + 63, the
dR pass over tile diagonals) and the 32 x 32 kernels of csrc/emo_softmax_attn32.hip, against the float64 references of tests/attn_ref.py
(gradients: autograd on them).

Every call runs on a GUARDED layout: qkv, R, dout, the biased query copies, out, lse, zden, delta, dqkv, dq_rel, dR and the dR workspace each live
inside a larger allocation.  The rows (and the pad columns of a padded row stride) around an input are NaN — one row too far ends in a NaN
result; the bands around an output hold a sentinel that must still be there afterwards, and the output itself, NaN before the call, must be
finite.  Each case runs with the packed row strides and with padded ones (qkv: 3 H dh + 8 elements).  The ops wrappers allocate out, lse and
zden themselves, so the cases drive ops._attn with the wrappers' own field lists.  H = 3, B = 2, sequence b's inputs scaled by (1 + b); every
comparison is made per sequence, against that sequence's own max-abs.

Tolerances are the project's (tests/test_gpu_kernels.py): 2e-5 fp32 / 3e-2 bf16 of the reference's max-abs, times 1 for out (and lse, zden),
3 for the softmax gradients (one scale over dq, dk, dv), 4 / 6 / 8 for the relpos dqkv / dR / bias gradients.  At T = 1 the reference's dR and
bias gradients vanish identically (one key: p = 1 whatever the scores); their scale is then the dqkv scale of the call — they are sums of the
same ds terms times operands of the same magnitude.  The SELECTOR cases are exact: tests/test_attn_ref_host.py proves their probabilities
one-hot in fp32, so an output row must equal a row of v bit for bit."""
import functools

import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
H3, B2 = 3, 2
GR = 64                                  # guard rows on either side of every buffer: a whole 64-row tile read past the end stays inside the allocation
SENT = 1536.0                            # the sentinel of the output guard bands (exact in bf16)
NAN = float('nan')
P_DROP, SEED, OFFSET = 0.25, 3, 9


def _ops():
    from emo_disentanger_amd import ops
    return ops


def _tol(dt):
    return 2e-5 if dt == F32 else 3e-2


def _name(dt):
    return 'f32' if dt == F32 else 'bf16'


def _close(got, ref, dt, what, mult=1.0, scale=None, floor=1e-6):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, what
    assert torch.isfinite(got).all(), '%s: not finite' % what
    s = max(float(ref.abs().max()) if scale is None else scale, floor)
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    print('[attn_train_edges] %s: err/scale %.3e (bound %.1e)' % (what, err / s, mult * _tol(dt)))
    assert err <= mult * _tol(dt) * s, '%s: max err %.3e vs scale %.3e (tol %.1e)' % (what, err, s, mult * _tol(dt))


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


# ------------------------------------------------------------------------------------------- guarded buffers
class _Buf:
    """[M, W] inside a [(M + 2 GR), ld] device allocation.  data given: an INPUT (everything around it NaN); else an OUTPUT (the core NaN, the
    bands and pad columns the sentinel)."""

    def __init__(self, M, W, ld, dt, data=None):
        assert ld >= W
        self.is_input = data is not None
        self.buf = torch.full((M + 2 * GR, ld), NAN if self.is_input else SENT, dtype=dt, device='cuda')
        self.core = self.buf[GR:GR + M, :W]
        self.core.copy_(data.to(dt).reshape(M, W) if self.is_input else torch.full((M, W), NAN, dtype=dt))
        self.before = self.buf.clone() if self.is_input else None
        self.inside = torch.zeros(M + 2 * GR, ld, dtype=torch.bool, device='cuda')
        self.inside[GR:GR + M, :W] = True

    def check(self, what):
        if self.is_input:
            assert torch.equal(_bits(self.buf), _bits(self.before)), '%s: an input changed' % what
        else:
            assert bool((self.buf[~self.inside] == SENT).all()), '%s: a store outside the output' % what
            assert bool(torch.isfinite(self.core).all()), '%s: not every element written, or not finite' % what


def _vec(n, data=None):
    """a flat fp32 vector with guard bands"""
    return _Buf(1, n, n, F32, data)


class _Bufs(dict):
    def check(self, what):
        for name, b in self.items():
            b.check('%s, %s' % (what, name))


def _rows(x):
    """[B, T, H, d] -> [B T, H d]"""
    return x.reshape(x.shape[0] * x.shape[1], -1)


# ------------------------------------------------------------------------------------------- launches (the field lists of the ops wrappers)
def _softmax(dt, q, k, v, dout=None, padded=False, p=0.0, want_keep=False, what=''):
    """q, k, v, dout [B, T, H, dh] (host, exact in dt) -> dict of host tensors: out, dq, dk, dv [B, T, H, dh] in dt, lse [B, H, T], keep"""
    ops = _ops()
    B, T, H, dh = q.shape
    M, HD, pad = B * T, H * dh, 8 if padded else 0
    bufs = _Bufs(qkv=_Buf(M, 3 * HD, 3 * HD + pad, dt, torch.cat([_rows(x) for x in (q, k, v)], 1)), out=_Buf(M, HD, HD + pad, dt), lse=_vec(B * H * T))
    c = bufs['qkv'].core
    qv, kv, vv = c[:, :HD], c[:, HD:2 * HD], c[:, 2 * HD:]
    keep, kbytes = None, 0
    if want_keep:
        kbytes = ops.lib.emo_softmax_attn_keep_bytes(ops.dtype_code(dt), B, T, H, dh, p)
        keep = torch.empty(kbytes // 4, device='cuda', dtype=torch.int32) if kbytes else None
    drop = dict(p_drop=p, seed=SEED, offset=OFFSET, keep=ops.ptr(keep), keep_bytes=kbytes)
    ops._attn(ops.ATTN_SOFTMAX, ops.ATTN_FWD, qv, kv, vv, B, T, H, out=ops.ptr(bufs['out'].core), ld_out=HD + pad, lse=ops.ptr(bufs['lse'].core), **drop)
    bufs.check(what + ' fwd')
    res = dict(out=bufs['out'].core.cpu().view(B, T, H, dh), lse=bufs['lse'].core.cpu().view(B, H, T), keep=keep)
    if dout is None:
        return res
    bufs.update(dout=_Buf(M, HD, HD + pad, dt, _rows(dout)), dqkv=_Buf(M, 3 * HD, 3 * HD + pad, dt), delta=_vec(B * H * T))
    bufs['out'].is_input, bufs['out'].before = True, bufs['out'].buf.clone()          # from here on out and lse are inputs
    bufs['lse'].is_input, bufs['lse'].before = True, bufs['lse'].buf.clone()
    g = bufs['dqkv'].core
    ops._attn(ops.ATTN_SOFTMAX, ops.ATTN_BWD, qv, kv, vv, B, T, H, out=ops.ptr(bufs['out'].core), dout=ops.ptr(bufs['dout'].core), ld_out=HD + pad,
              lse=ops.ptr(bufs['lse'].core), delta_ws=ops.ptr(bufs['delta'].core), dq=ops.ptr(g[:, :HD]), dk=ops.ptr(g[:, HD:2 * HD]), dv=ops.ptr(g[:, 2 * HD:]),
              ld_d=3 * HD + pad, **drop)
    bufs.check(what + ' bwd')
    gh = g.cpu()
    res.update(dq=gh[:, :HD].reshape(B, T, H, dh), dk=gh[:, HD:2 * HD].reshape(B, T, H, dh), dv=gh[:, 2 * HD:].reshape(B, T, H, dh))
    return res


def _relpos(dt, q, k, v, R, u, vb, dout=None, padded=False, p=0.0, window=0, what='', over=None):
    """As _softmax; R [T, H, dh], u, vb [H, dh].  -> out, lse, zden and, with dout, dq, dk, dv, dR [T, H, dh] fp32, du, dvb [H, dh] fp32.
    over: pass name -> fields that replace the call's own (the refusal cases)."""
    ops = _ops()
    over = over or {}
    B, T, H, dh = q.shape
    M, HD, pad = B * T, H * dh, 8 if padded else 0
    bufs = _Bufs(qkv=_Buf(M, 3 * HD, 3 * HD + pad, dt, torch.cat([_rows(x) for x in (q, k, v)], 1)), R=_Buf(T, HD, HD + pad, dt, R.reshape(T, HD)),
                 out=_Buf(M, HD, HD + pad, dt), lse=_vec(B * H * T), zden=_vec(B * H * T))
    ud, vbd = u.float().cuda().contiguous(), vb.float().cuda().contiguous()
    c = bufs['qkv'].core
    qv, kv, vv = c[:, :HD], c[:, HD:2 * HD], c[:, 2 * HD:]
    shared = dict(r_dist=ops.ptr(bufs['R'].core), ld_r=HD + pad, n_dist=T, lse=ops.ptr(bufs['lse'].core), zden=ops.ptr(bufs['zden'].core), p_drop=p, seed=SEED,
                  offset=OFFSET)
    bias = dict(r_w_bias=ops.ptr(ud), r_r_bias=ops.ptr(vbd))
    f = dict(shared, out=ops.ptr(bufs['out'].core), ld_out=HD + pad, window=int(window), **bias)
    f.update(over.get('fwd', {}))
    ops._attn(ops.ATTN_RELPOS, ops.ATTN_FWD, qv, kv, vv, B, T, H, **f)
    bufs.check(what + ' fwd')
    res = dict(out=bufs['out'].core.cpu().view(B, T, H, dh), lse=bufs['lse'].core.cpu().view(B, H, T), zden=bufs['zden'].core.cpu().view(B, H, T))
    if dout is None:
        return res
    for name in ('out', 'lse', 'zden'):
        bufs[name].is_input, bufs[name].before = True, bufs[name].buf.clone()
    bufs.update(dout=_Buf(M, HD, HD + pad, dt, _rows(dout)), dqkv=_Buf(M, 3 * HD, 3 * HD + pad, dt), dq_rel=_Buf(M, HD, HD + pad, dt), delta=_vec(B * H * T))
    g = bufs['dqkv'].core
    common = dict(shared, dout=ops.ptr(bufs['dout'].core), ld_out=HD + pad, delta=ops.ptr(bufs['delta'].core), ld_d=3 * HD + pad)
    f = dict(common, out=ops.ptr(bufs['out'].core), dq=ops.ptr(g[:, :HD]), dq_rel=ops.ptr(bufs['dq_rel'].core), ld_rel=HD + pad, **bias)
    f.update(over.get('bwd', {}))
    ops._attn(ops.ATTN_RELPOS, ops.ATTN_BWD, qv, kv, vv, B, T, H, **f)
    # the key-tile and distance-window passes read the biased query copies in the place of q
    qu_c, qv_c = ops.add_bias2(qv, ud, vbd)
    bufs.update(qu=_Buf(M, HD, HD + pad, dt, qu_c), qvb=_Buf(M, HD, HD + pad, dt, qv_c))
    bufs['delta'].check(what + ' bwd, delta')
    bufs['delta'].is_input, bufs['delta'].before = True, bufs['delta'].buf.clone()
    common.update(qu=ops.ptr(bufs['qu'].core), qv=ops.ptr(bufs['qvb'].core), ld_q=HD + pad)
    f = dict(common, dk=ops.ptr(g[:, HD:2 * HD]), dv=ops.ptr(g[:, 2 * HD:]))
    f.update(over.get('bwd_kv', {}))
    ops._attn(ops.ATTN_RELPOS, ops.ATTN_BWD_KV, bufs['qu'].core, kv, vv, B, T, H, **f)
    ws_bytes = ops.lib.emo_relpos_attn_bwd_r_workspace_bytes(B, T, H, dh)
    bufs.update(dR=_Buf(T, HD, HD + (4 if padded else 0), F32), ws=_vec(ws_bytes // 4))
    f = dict(common, dR=ops.ptr(bufs['dR'].core), ld_dr=HD + (4 if padded else 0), workspace=ops.ptr(bufs['ws'].core), workspace_bytes=ws_bytes)
    f.update(over.get('bwd_r', {}))
    ops._attn(ops.ATTN_RELPOS, ops.ATTN_BWD_R, bufs['qu'].core, kv, vv, B, T, H, **f)
    bufs.check(what + ' bwd')
    d_rr = ops.colsum(bufs['dq_rel'].core)
    d_rw = ops.colsum(g[:, :HD]) - d_rr
    gh = g.cpu()
    res.update(dq=gh[:, :HD].reshape(B, T, H, dh), dk=gh[:, HD:2 * HD].reshape(B, T, H, dh), dv=gh[:, 2 * HD:].reshape(B, T, H, dh),
               dR=bufs['dR'].core.cpu().view(T, H, dh), du=d_rw.cpu().view(H, dh), dvb=d_rr.cpu().view(H, dh))
    return res


# ------------------------------------------------------------------------------------------- inputs and references (one per case, shared)
def _r(*shape, seed=0, dt=F32, scale=1.0):
    """randn rounded to dt, sequence b (the first dimension of a [B, T, H, dh] tensor) scaled by (1 + b), as float64"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g) * scale
    if len(shape) == 4:
        x = x * (1 + torch.arange(shape[0], dtype=torch.float32))[:, None, None, None]
    return x.to(dt).double()


def _mask(B, T, H, p):
    if p <= 0:
        return None
    from dropmask import site_multipliers
    n = B * H * T * T                                              # (the read-out takes multiples of 4 elements; the index is the flat one)
    return site_multipliers(((n + 3) // 4 * 4,), p, SEED, OFFSET)[:n].view(B, H, T, T).double()


@functools.lru_cache(maxsize=None)
def _softmax_case(dt, B, T, H, dh, p):
    q, k, v, dout = [_r(B, T, H, dh, seed=s, dt=dt) for s in (11, 12, 13, 14)]
    leaf = [x.clone().requires_grad_(True) for x in (q, k, v)]
    out, lse = ar.softmax_ref(*leaf, mask=_mask(B, T, H, p))
    out.backward(dout)
    return (q, k, v, dout), dict(out=out.detach(), lse=lse.detach(), dq=leaf[0].grad, dk=leaf[1].grad, dv=leaf[2].grad)


@functools.lru_cache(maxsize=None)
def _relpos_case(dt, B, T, H, dh, p):
    q, k, v = [_r(B, T, H, dh, seed=s, dt=dt, scale=0.7) for s in (21, 22, 23)]
    dout = _r(B, T, H, dh, seed=24, dt=dt)
    R, u, vb = _r(T, H, dh, seed=25, dt=dt, scale=0.7), _r(H, dh, seed=26, scale=0.3), _r(H, dh, seed=27, scale=0.3)
    leaf = [x.clone().requires_grad_(True) for x in (q, k, v, R, u, vb)]
    out, lse, zden = ar.relpos_ref(*leaf, mask=_mask(B, T, H, p))
    out.backward(dout)
    ref = dict(out=out.detach(), lse=lse.detach(), zden=zden.detach())
    ref.update({n: leaf[i].grad for i, n in enumerate(('dq', 'dk', 'dv', 'dR', 'du', 'dvb'))})
    return (q, k, v, R, u, vb, dout), ref


def _check_softmax(got, ref, dt, what):
    B = ref['out'].shape[0]
    for b in range(B):
        w = '%s, sequence %d' % (what, b)
        _close(got['out'][b], ref['out'][b], dt, w + ', out')
        _close(got['lse'][b], ref['lse'][b], dt, w + ', lse')
        gs = max(float(ref[n][b].abs().max()) for n in ('dq', 'dk', 'dv'))
        for n in ('dq', 'dk', 'dv'):
            _close(got[n][b], ref[n][b], dt, '%s, %s' % (w, n), mult=3, scale=gs)


def _check_relpos(got, ref, dt, what, fwd_only=False):
    B, T = ref['out'].shape[:2]
    for b in range(B):
        w = '%s, sequence %d' % (what, b)
        _close(got['out'][b], ref['out'][b], dt, w + ', out')
        _close(got['lse'][b], ref['lse'][b], dt, w + ', lse')
        _close(got['zden'][b], ref['zden'][b], dt, w + ', zden')
        if not fwd_only:
            gs = max(float(ref[n][b].abs().max()) for n in ('dq', 'dk', 'dv'))
            for n in ('dq', 'dk', 'dv'):
                _close(got[n][b], ref[n][b], dt, '%s, %s' % (w, n), mult=4, scale=gs)
    if not fwd_only:
        floor = max(float(ref[n].abs().max()) for n in ('dq', 'dk', 'dv')) if T == 1 else 1e-6
        _close(got['dR'], ref['dR'], dt, what + ', dR', mult=6, floor=floor)
        _close(got['du'], ref['du'], dt, what + ', du', mult=8, floor=floor)
        _close(got['dvb'], ref['dvb'], dt, what + ', dvb', mult=8, floor=floor)


# ------------------------------------------------------------------------------------------- the generic kernels against float64
EDGE_T = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 191, 193)
SHAPES = [(T, 64) for T in EDGE_T] + [(T, dh) for dh in (16, 32) for T in (17, 65, 129)]
GENERIC = [(dt, T, dh, False) for dt in DT for T, dh in SHAPES] + [(BF16, T, 64, True) for T in (128, 256)]
_ids = lambda cases: ['%s-T%d-dh%d%s' % (_name(c[0]), c[1], c[2], '-generic' if c[3] else '') for c in cases]


@pytest.mark.parametrize('dt,T,dh,force', GENERIC, ids=_ids(GENERIC))
def test_softmax_forward_and_backward_at_tile_edges(dt, T, dh, force, monkeypatch):
    """sattn_fwd_kernel, sattn_bwd_dq_kernel, sattn_bwd_dkv_kernel: T on both sides of a wave (16 rows) and of a tile (64 rows), one key, and the
    bf16 / d_head 64 / T % 128 == 0 shapes with the 32 x 32 kernels switched off."""
    if force:
        monkeypatch.setenv('EMO_SATTN32', '0')
    inp, ref = _softmax_case(dt, B2, T, H3, dh, 0.0)
    for padded in (False, True):
        what = 'softmax %s T=%d dh=%d%s' % (_name(dt), T, dh, ' padded' if padded else '')
        _check_softmax(_softmax(dt, *inp, padded=padded, what=what), ref, dt, what)


@pytest.mark.parametrize('dt,T,dh,force', GENERIC[:-2], ids=_ids(GENERIC[:-2]))
def test_relpos_forward_and_backward_at_tile_edges(dt, T, dh, force):
    """relattn_fwd_kernel, relattn_bwd_kernel, relattn_bwd_dkv_kernel, relattn_bwd_dr_kernel, relattn_dr_reduce_kernel at the same lengths"""
    inp, ref = _relpos_case(dt, B2, T, H3, dh, 0.0)
    for padded in (False, True):
        what = 'relpos %s T=%d dh=%d%s' % (_name(dt), T, dh, ' padded' if padded else '')
        _check_relpos(_relpos(dt, *inp[:6], dout=inp[6], padded=padded, what=what), ref, dt, what)


@pytest.mark.parametrize('dt', DT, ids=_name)
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('T', [64, 65, 128, 129, 193])
def test_relpos_dr_pass_sums_diagonals_and_batch_in_a_fixed_order(dt, B, T):
    """1, 2, 2, 3 and 4 tile diagonals: every distance past 0 is covered by two overlapping 128-distance windows, summed over the batch by
    relattn_dr_reduce_kernel in a fixed order — the pass is documented as deterministic, so two runs are bit-identical."""
    inp, ref = _relpos_case(dt, B, T, H3, 64, 0.0)
    what = 'relpos dR %s B=%d T=%d' % (_name(dt), B, T)
    a = _relpos(dt, *inp[:6], dout=inp[6], padded=True, what=what)
    b = _relpos(dt, *inp[:6], dout=inp[6], padded=True, what=what)
    assert torch.equal(a['dR'], b['dR']), what
    _check_relpos(a, ref, dt, what)


# ------------------------------------------------------------------------------------------- dropout on
@pytest.mark.parametrize('dt', DT, ids=_name)
@pytest.mark.parametrize('T', [17, 65, 68, 129])
@pytest.mark.parametrize('kind', ['softmax', 'relpos'])
def test_dropout_on_at_tile_edges(kind, T, dt):
    """p = 0.25 with the multipliers read out of the library (dropmask.site_multipliers over the flat site of B H T T elements, element
    ((b H + h) T + i) T + j): out and every gradient against the float64 reference under that mask.  T = 68 next to the odd lengths: T % 4 == 0
    is where the dK/dV kernels hash one word per four rows (drop_mult_col4) instead of one per element."""
    for padded in (False, True):
        what = '%s dropout %s T=%d%s' % (kind, _name(dt), T, ' padded' if padded else '')
        if kind == 'softmax':
            inp, ref = _softmax_case(dt, B2, T, H3, 64, P_DROP)
            _check_softmax(_softmax(dt, *inp, padded=padded, p=P_DROP, what=what), ref, dt, what)
        else:
            inp, ref = _relpos_case(dt, B2, T, H3, 64, P_DROP)
            _check_relpos(_relpos(dt, *inp[:6], dout=inp[6], padded=padded, p=P_DROP, what=what), ref, dt, what)


# ------------------------------------------------------------------------------------------- the 32 x 32 kernels against float64
@pytest.mark.parametrize('T,p', [(128, 0.0), (256, 0.0), (384, 0.0), (256, P_DROP)])
def test_softmax_32x32_kernels_against_float64(T, p, monkeypatch):
    """out, lse, dQ, dK and dV of the 32 x 32 kernels (bf16, d_head 64, T % 128 == 0) each against float64.  That these kernels served the call:
    with dropout the keep words exist (a forward the generic kernels serve refuses them); without, the result differs bitwise from the
    EMO_SATTN32=0 run."""
    dt = BF16
    inp, ref = _softmax_case(dt, B2, T, H3, 64, p)
    for padded in (False, True):
        what = 'softmax 32x32 T=%d p=%.2f%s' % (T, p, ' padded' if padded else '')
        got = _softmax(dt, *inp, padded=padded, p=p, want_keep=p > 0, what=what)
        _check_softmax(got, ref, dt, what)
        if p > 0:
            assert got['keep'] is not None, what
        else:
            monkeypatch.setenv('EMO_SATTN32', '0')
            gen = _softmax(dt, *inp, padded=padded, what=what + ' (generic)')
            monkeypatch.delenv('EMO_SATTN32')
            # per pass: forward (out, lse), dQ, dK/dV.  (A bf16 tensor alone can agree bit for bit by chance: the two kernel sets differ by fp32
            # reassociation, which flips few bf16 roundings; at T = 128 `out` does agree, lse does not.)
            same = {n: torch.equal(_bits(got[n]), _bits(gen[n])) for n in ('out', 'lse', 'dq', 'dk', 'dv')}
            print('[attn_train_edges] %s: bit-identical to the generic kernels: %s' % (what, [n for n in same if same[n]]))
            assert not (same['out'] and same['lse']), what + ': the forward is bit-identical to the generic kernels'
            assert not same['dq'], what + ': dQ is bit-identical to the generic kernels'
            assert not (same['dk'] and same['dv']), what + ': dK / dV are bit-identical to the generic kernels'


# ------------------------------------------------------------------------------------------- selector inputs: exact results
def _softmax_selector_case(dt, T, dh, what):
    maps = ar.selector_maps(T)
    for names in ar.SEL_MAPS:
        pis = [maps[n] for n in names]
        q, k, v = ar.softmax_selector(B2, T, H3, dh, pis, seed=T + dh)
        dout = ar.small_int_dout(B2, T, H3, dh, seed=T)
        want_lse = torch.full((B2, H3, T), ar.G * dh / dh ** 0.5, dtype=torch.float64)
        want_dv = ar.softmax_selector_dv(dout, pis).to(dt)
        for padded in (False, True):
            w = '%s %s%s' % (what, '/'.join(names), ' padded' if padded else '')
            got = _softmax(dt, q, k, v, dout=dout, padded=padded, what=w)
            for h, pi in enumerate(pis):
                assert torch.equal(got['out'][:, :, h], v[:, pi, h].to(dt)), '%s: head %d (%s), an output row is not its key\'s v row' % (w, h, names[h])
            _close(got['lse'], want_lse, F32, w + ', lse')
            assert torch.equal(got['dv'], want_dv), w + ': dv is not the integer sum of dout over pi(i) = j'
            assert not got['dq'].any() and not got['dk'].any(), w + ': dq / dk not exactly 0'


@pytest.mark.parametrize('dt', DT, ids=_name)
@pytest.mark.parametrize('T,dh', ar.SEL_GENERIC)
def test_softmax_selector_on_the_generic_kernels(T, dh, dt):
    """Every probability is exactly 0 or 1 (tests/test_attn_ref_host.py): out[b, i, h] EQUALS v[b, pi(i), h] for pi = the diagonal, key 0, the
    first key of the row's tile, the last keys of the previous tile (i - 64, i - 65) and a pseudo-random key; lse within the fp32 bound (the
    statistics live in the base-2 domain); with integer dout, dv EQUALS the integer sum (a bf16 dv: its one rounding) and dq = dk = 0."""
    _softmax_selector_case(dt, T, dh, 'softmax selector %s T=%d dh=%d' % (_name(dt), T, dh))


@pytest.mark.parametrize('T,dh', ar.SEL_FUSED32)
def test_softmax_selector_on_the_32x32_kernels(T, dh):
    """The same on the 32 x 32 forward, dQ and dK/dV kernels (test_softmax_32x32_kernels_against_float64 shows they serve these layouts)"""
    _softmax_selector_case(BF16, T, dh, 'softmax selector 32x32 T=%d' % T)


@pytest.mark.parametrize('dt', DT, ids=_name)
@pytest.mark.parametrize('T', ar.SEL_RELPOS_T)
def test_relpos_selector_distances_and_windows(T, dt):
    """q = k = 0, vb = e_0, R[d*][h, 0] = G: row i >= d* selects key i - d* — out EQUALS that v row and zden EQUALS fp32(1 + 1e-8) — for d* at the
    skew buffer's ends (0, 79 / 80, 127 / 128), on both sides of a key-tile step (63 / 64 / 65, 15 / 16) and at the last distance of the table
    (T - 1); the other rows are uniform and meet relpos_ref at the usual bound.  Again on the banded forward with window = d* (the key inside
    the band) and d* - 1 (just outside: uniform over the band).  Equality, not one ulp: the kernel's last operation is
    `inv = 1.f / (e_run + 1e-8f * l_run)` (relattn_fwd_kernel, csrc/emo_softmax_attn.hip), an IEEE division (no fast-math flag in
    csrc/Makefile) of 1 by fp32(1 + 1e-8) = 1, and zden is e_run / l_run + 1e-8f = 1 / 1 + 1e-8f."""
    B, H, dh = B2, H3, ar.SEL_RELPOS_DH
    one = torch.ones(1)
    for dstar in ar.relpos_dstar(T):
        q, k, v, R, u, vb = ar.relpos_selector(B, T, H, dh, dstar, seed=T)
        for w in ar.relpos_windows(dstar):
            sel = ar.relpos_selected(T, dstar, w)
            ref = dict(zip(('out', 'lse', 'zden'), ar.relpos_ref(q, k, v, R, u, vb, window=w)))
            for padded in (False, True):
                what = 'relpos selector %s T=%d d*=%s window=%d%s' % (_name(dt), T, dstar, w, ' padded' if padded else '')
                got = _relpos(dt, q, k, v, R, u, vb, padded=padded, window=w, what=what)
                for h in range(H):
                    rows = torch.nonzero(sel[h] >= 0)[:, 0]
                    assert torch.equal(got['out'][:, rows, h], v[:, sel[h, rows], h].to(dt)), '%s: head %d, a row is not the v row at distance %d' % (what, h, dstar[h])
                    assert torch.equal(got['zden'][:, h, rows], one.expand(B, len(rows))), '%s: head %d, zden' % (what, h)
                _check_relpos(got, ref, dt, what, fwd_only=True)


# ------------------------------------------------------------------------------------------- refusals
def test_calls_the_training_passes_do_not_serve_raise():
    ops = _ops()
    B, T, H = 1, 20, 1
    # d_head 128: built for the decode passes only
    x = torch.zeros(B * T, 3 * 128, device='cuda')
    o, lse = torch.full((B * T, 128), NAN, device='cuda'), torch.full((B, H, T), NAN, device='cuda')
    q, k, v = x[:, :128], x[:, 128:256], x[:, 256:]
    with pytest.raises(RuntimeError, match='d_head'):
        ops.softmax_attn_fwd(q, k, v, B, T, H)
    with pytest.raises(RuntimeError, match='d_head'):
        ops.softmax_attn_bwd(q, k, v, torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(lse), B, T, H)
    R, u = torch.zeros(T, 128, device='cuda'), torch.zeros(H, 128, device='cuda')
    with pytest.raises(RuntimeError, match='d_head'):
        ops.relpos_attn_fwd(q, k, v, R, u, u, B, T, H)
    with pytest.raises(RuntimeError, match='d_head'):
        ops.relpos_attn_bwd(x, R, u, u, torch.zeros_like(o), torch.zeros_like(o), torch.zeros_like(lse), torch.ones_like(lse), B, T, H)
    # the relpos checks, on a problem every pass serves
    inp, _ = _relpos_case(F32, 1, 20, H3, 16, 0.0)
    args, dout = inp[:6], inp[6]
    with pytest.raises(RuntimeError, match='r_dist needs a row'):
        _relpos(F32, *args, over={'fwd': dict(n_dist=19)})                                  # n_dist < T without a window
    _relpos(F32, *args, window=5, over={'fwd': dict(n_dist=6)})                           # (with one, min(T, W + 1) rows are enough)
    with pytest.raises(RuntimeError, match='r_dist needs a row'):
        _relpos(F32, *args, window=5, over={'fwd': dict(n_dist=5)})
    with pytest.raises(RuntimeError, match='p_drop must be 0'):
        _relpos(F32, *args, window=5, p=P_DROP)                                            # a window with dropout on
    with pytest.raises(RuntimeError, match='window'):
        _relpos(F32, *args, dout=dout, over={'bwd': dict(window=5)})                        # the backward passes are not windowed
    need = ops.lib.emo_relpos_attn_bwd_r_workspace_bytes(1, 20, H3, 16)
    assert need == 1 * H3 * 1 * 128 * 16 * 4
    with pytest.raises(RuntimeError, match='workspace too small'):
        _relpos(F32, *args, dout=dout, over={'bwd_r': dict(workspace_bytes=need - 1)})     # a dR workspace one byte too small
    _relpos(F32, *args, dout=dout)
