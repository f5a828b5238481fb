"""The FAVOR+ training kernels (csrc/emo_favor.hip, csrc/emo_favor_fs.hip: forward, dq sweep, dk/dv sweep) at their chunk and segment edges,
element by element against the float64 reference tests/favor_ref.py evaluated on the inputs as the kernel receives them (bf16 inputs are upcast
exactly).  B = 2 streams and H = 3 heads unless noted: three heads keep `/ H` and `% H` from hiding behind a power of two, two streams put
stream 1 off the chunk grid whenever T is.  Kernel families: `f32` (generic kernels, exact-f32 MFMA; chunks 32 / 32 / 16 tokens for forward / dq
/ dk,dv at d_head 64 and 32 elsewhere), `bf16` (generic kernels, EMO_FAVOR_FS=0; chunks of 64), `fs` (the slice kernels, EMO_FAVOR_FS=2; bf16,
d_head 64, 128 features, chunks of 32).  The case lists below are shared with tests/test_favor_ref_host.py, which shows on the CPU that a float32
and a bf16-emulated evaluation of the reference stay inside these bounds at every case and that every seeded defect breaks them at a named case.

The bound (favor_ref.Bounds), per element:   |got - ref| <= u (k mag + mag_rho) + mag_in + u_store |ref| + 2^-80
  mag      the magnitude companion: the same sums over absolute values of their terms (phi > 0, so |v|, |dN|, |dD|, |omega|, |x|)
  u        2^-24 (f32) / 2^-8 (bf16, fs): the unit round-off of the MFMA operands;  u_store = u: the rounding of out, dq, dk, dv (0 for den, S, z)
  k        the roundings an operand chain passes through, counted below
  mag_rho  the companion with phi(x) replaced by phi(x) expm1(u rho(x)) / u, once for q and once for k (and u times both): rho is the error of
           the exp's ARGUMENT in units of u.  With A = sum_d |c x_d omega_dm| and off = |c x|^2 / 2 + ln(F) / 2:
             bf16, fs: rho = A + 2^-15 (dh + 6)(A + off).  The kernels round omega to bf16 (WT = from_f32<CT>(omega)), which moves u = (c x) omega
                       by up to 2^-8 A; the second term is the float32 arithmetic of f32 below in units of 2^-8, doubled for the slice kernels'
                       log2(e)-scaled argument of exp2.
             f32:      rho = (dh + 6)(A + off) + 4.  u is an fp32 sum of dh products times c (<= (dh + 2) 2^-24 A), off an fp32 sum of dh
                       squares ((dh + 3) 2^-24 off), the subtraction rounds once (2^-24 (A + off)), expf is good to 2 ulp (4 x 2^-24).
  mag_in   the companion of the gradients with (|dN|, |dD|) replaced by the bounds of THEIR errors: the backward reads the kernel's own den and the
           STORED out, so dN inherits den's relative bound r (and its own rounding u_g: one bf16 rounding, 2 x 2^-24 in f32, none in the
           dout_is_dn form where dN is an input), dD inherits sum_d |dout_d| bound(out_d) / den, r, and u_dd (one bf16 rounding in the slice
           kernels, which feed dD to an MFMA; 2^-16 x 2^-8 >= (dh + 3) 2^-24 elsewhere).  k and mag_rho are applied to |dN| + err, |dD| + err.
  2^-80    products under 2^-126 may flush to zero: at most T F of them per sum, divided by den >= eps.

The counts k.  `+ 0.5` stands for all float32 accumulation on a bf16 path: sums of at most T + F + 16 <= 592 terms (the segmented scan adds
one fp32 sum over at most 16 increments), 592 x 2^-24 < 0.01 x 2^-8.  On the f32 path every chain is bounded by its length instead,
n = F + T + dh + 16 (any summation order of n terms errs by at most n u sum|terms|; the 16 are the segment sum).
  num (numerator of out)  bf16, fs: phi(q) 1, phi(k) 1, then either the masked chunk matrix A rounded as an operand (1) or the carried state's bf16
       mirror (1): 3.5.  f32: the feature dot (F) and the sum over tokens (T): n.
  den  as num: the row sums are taken over the ROUNDED A, z is carried in fp32 from rounded features (the slice kernels carry z through the MFMA
       with S, so their z passes through the mirror rounding as S does): 3.5; f32: n.   out = num / den: (bound(num) + |out| bound(den)) / (den (1 - r)).
  S, z  rounded phi(k) times the exact v, fp32 sums: 1.5; f32: n.
  dv   dN (in mag_in), then phi(q) 1, phi(k) 1, A or the R mirror 1: 3.5; the slice kernels fold 1 / den into a second rounding of phi(q)^T: 4.5; f32: n.
  dq, dk  P = dN.v + dD rounded as an operand 1 (or the S / R mirror 1), the other side's features 1, own features 1 (a = dPhi * phi), Adiff
       rounded as the operand of the omega product 1, omega 1: 5.5; the slice kernels round dD once more before P is formed: 6.5;
       f32: the P / state chain and the omega product: 2 n.

Observed max err / bound on the MI355X (worst case of each family over every case of this file; the tests print them):
                      out    den    S      z      dq     dk     dv
    f32               0.022  0.030  0.049  0.043  0.003  0.002  0.017
    bf16              0.118  0.225  0.427  0.427  0.016  0.034  0.158
    fs                0.108  0.139  0.248  0.209  0.016  0.007  0.065
    fs, dout_is_dn    0.077  0.115  0.248  0.209  0.007  0.014  0.171
    fs into bf16 bwd  0.066  0.122  0.180  0.143  0.004  0.007  0.056
Most of the slack is the omega term: rho = A is the worst case over the signs of dh roundings, A is about 11 at d_head 64.

Found by this file: the fp32 dq and dk of two identical calls differed in their last bits (13 cases, all f32 at d_head 64: two identical calls,
dq[:t0] in the causality cases, recomputed against kept K-state).  jac_epilogue added each 16-feature tile's share of the Jacobian's row sum with
atomicAdd into one LDS float per row, in the order the waves arrived; it now stores one slot per tile and dx_from_adiff sums them in tile order.
The `pos` class (v, dout > 0) makes dD = -(dN.out) a sum without cancellation: with random signs a wrongly scaled dD of the dout_is_dn form moves
less than the bound that the error of `out` puts on dD itself (tests/test_favor_ref_host.py, dd_from_dout_in_dn_form).

The loud-token scale (case class `loud`): LOUD_SCALE is the largest of {2, 3, 4, 6} at which the float32 and the bf16-emulated evaluations of the
reference are finite and inside the bound (tests/test_favor_ref_host.py asserts that it is)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import favor_ref as R

pytestmark = pytest.mark.gpu

B_, H_ = 2, 3
PAIRS = [(64, 128), (32, 128), (32, 64), (16, 32), (16, 64)]
T_EDGE = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129]
LOUD_SCALE = 6
LOUD_ROWS = (0, 1, 20, 21)
FAMS = ('f32', 'bf16', 'fs')


def chunks(fam, dh):
    """(forward, dq, dk/dv) chunk sizes: csrc/emo_favor.hip dispatch_favor, csrc/emo_favor_fs.hip FS_C"""
    return (32, 32, 32) if fam == 'fs' else (64, 64, 64) if fam == 'bf16' else (32, 32, 16) if dh == 64 else (32, 32, 32)


def seg_len(T, want):
    """csrc/emo_favor.hip favor_segments: (segments, tokens per segment)"""
    want = max(1, min(want, 16, T // 128))
    Ts = max(64, -(-(-(-T // want)) // 64) * 64)
    return -(-T // Ts), Ts


def case(fam, T, dh=64, nf=128, segs=1, eps=1e-6, cls='plain', fs_bwd=True, dn=False, B=B_, H=H_):
    return dict(fam=fam, T=T, dh=dh, nf=nf, segs=segs, eps=eps, cls=cls, fs_bwd=fs_bwd, dn=dn, B=B, H=H)


def key(c):
    return '-'.join('%s' % c[x] for x in ('fam', 'T', 'dh', 'nf', 'segs', 'eps', 'cls')) + ('' if c['fs_bwd'] else '-genbwd') + ('-dn' if c['dn'] else '')


SEGMENTED = [(256, 2, 2), (257, 2, 2), (400, 3, 3), (300, 16, 2)]        # (T, EMO_FAVOR_SEGMENTS, the segments the geometry gives)
CASES_A = {(fam, dh, nf): [case(fam, T, dh, nf) for T in T_EDGE] for fam in ('f32', 'bf16') for dh, nf in PAIRS}
CASES_B = [case(fam, T, dh, nf, segs=s) for fam in ('f32', 'bf16') for dh, nf in ((64, 128), (16, 32)) for T, s, _ in SEGMENTED]
CASES_C = ([case('fs', T) for T in (32, 64, 96, 160)] + [case('fs', 256, segs=2), case('fs', 288, segs=2)] +
           [case('fs', 96, fs_bwd=False), case('fs', 256, segs=2, fs_bwd=False)] + [case('fs', 32, dn=True), case('fs', 96, dn=True), case('fs', 96, dn=True, cls='pos')])
CASES_D = [case(fam, T, eps=eps, cls=cls, dn=dn) for eps, cls in ((0.25, 'plain'), (0.0, 'eps0'))
           for fam, T, dn in (('f32', 65, False), ('bf16', 65, False), ('fs', 96, False), ('fs', 96, True))]
CASES_E = [case('f32', 65, cls='loud'), case('bf16', 65, cls='loud'), case('fs', 96, cls='loud')]
ALL_CASES = [c for cs in CASES_A.values() for c in cs] + CASES_B + CASES_C + CASES_D + CASES_E


def k_counts(c):
    fam = c['fam']
    if fam == 'f32':
        n = c['nf'] + c['T'] + c['dh'] + 16
        return dict(num=n, den=n, S=n, z=n, dv=n, dq=2 * n, dk=2 * n)
    gen = fam == 'bf16' or not c['fs_bwd']
    return dict(num=3.5, den=3.5, S=1.5, z=1.5, dv=3.5 if gen else 4.5, dq=5.5 if gen else 6.5, dk=5.5 if gen else 6.5)


def rho(c, omega):
    dh = c['dh']

    def f(x):
        A, off = R.arg_sizes(x, omega)
        return (dh + 6) * (A + off) + 4 if c['fam'] == 'f32' else A + 2.0 ** -15 * (dh + 6) * (A + off)
    return f


def omega_of(dh, nf):
    from oracle.weights import orthogonal_omega
    return orthogonal_omega(dh, nf, np.random.default_rng(5)).float().contiguous()


def make_inputs(c, seed=0, loud=LOUD_SCALE):
    """q, k, v, dout [B, T, H, dh] float64 (bf16-representable for the bf16 families) and omega float32; deterministic on the CPU"""
    B, T, H, dh = c['B'], c['T'], c['H'], c['dh']
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + dh + c['nf'])
    sc = {'eps0': 0.5, 'quiet': 0.3}.get(c['cls'], 0.8)
    q, k, v = [torch.randn(B, T, H, dh, generator=g) * sc for _ in range(3)]
    dout = torch.randn(B, T, H, dh, generator=g)
    if c['cls'] == 'pos':                                          # v, dout > 0: out > 0 and dD = -(dN.out) is a sum without cancellation
        v, dout = v.abs(), dout.abs()
    if c['cls'] == 'loud':
        rows = [t for t in LOUD_ROWS if t < T]
        q[:, rows] *= loud
        k[:, rows] *= loud
    if c['fam'] != 'f32':
        q, k, v, dout = [t.bfloat16().float() for t in (q, k, v, dout)]
    return [t.double() for t in (q, k, v, dout)] + [omega_of(dh, c['nf'])]


def dn_of(dout, den):
    """dN as the GEMM epilogue forms it (emo_epilogue_t.hdiv): fp32 quotient, one rounding to bf16.  dout [B,T,H,dh], den [B,H,T]"""
    return (dout.float() / den.float().permute(0, 2, 1).unsqueeze(-1)).bfloat16()


def bounds_of(c, q, k, v, dout, om, den_for_dn=None):
    """The reference and its bounds.  dout_is_dn cases: `dout` is replaced by dN formed from den_for_dn (default: the reference's den)"""
    u = 2.0 ** -24 if c['fam'] == 'f32' else 2.0 ** -8
    if c['dn']:
        den = R.forward(q, k, v, om.double(), c['eps'])['den'] if den_for_dn is None else den_for_dn
        dout = dn_of(dout, den).double()
    f32 = c['fam'] == 'f32'
    gen = c['fam'] != 'fs' or not c['fs_bwd']
    return R.Bounds(q, k, v, om.double(), dout, c['eps'], k_counts(c), u, rho(c, om.double()), u, 2 * u if f32 else u, u * 2.0 ** -16 if gen else u, dn=c['dn'])


@functools.lru_cache(maxsize=None)
def _cached(k_, seed):
    c = {kk: vv for kk, vv in k_}
    ins = make_inputs(c, seed)
    return ins, (None if c['dn'] else bounds_of(c, *ins))


def inputs_and_bounds(c, seed=0):
    return _cached(tuple(sorted(c.items())), seed)


# ---------------------------------------------------------------------------------------------------- the device side
def _ops():
    from emo_disentanger_amd import ops
    return ops


def _env(mp, c):
    if c['fam'] == 'fs' and not c['fs_bwd']:                       # mixed: the slice forward by the library's own choice, the generic backward
        mp.delenv('EMO_FAVOR_FS', raising=False)
    else:
        mp.setenv('EMO_FAVOR_FS', '2' if c['fam'] == 'fs' else '0')
    mp.setenv('EMO_FAVOR_SEGMENTS', str(c['segs']))
    if c['fs_bwd']:
        mp.delenv('EMO_FAVOR_FS_BWD', raising=False)
    else:
        mp.setenv('EMO_FAVOR_FS_BWD', '0')


def _dt(c):
    return torch.float32 if c['fam'] == 'f32' else torch.bfloat16


def _n_segments(c):
    ops = _ops()
    b = ops.lib.emo_favor_attn_workspace_bytes(c['B'], c['T'], c['H'], c['dh'], c['nf'])
    return max(1, b // (4 * c['B'] * c['H'] * (c['nf'] * c['dh'] + c['nf'])))


def _dev(c, q, k, v, dout, om):
    B, T, H, dh = q.shape
    dt = _dt(c)
    qkv = torch.cat([t.reshape(B * T, H * dh) for t in (q, k, v)], 1).to(dt).cuda().contiguous()
    return qkv, dout.reshape(B * T, H * dh).to(dt).cuda().contiguous(), om.cuda()


def run(c, q, k, v, dout, om, backward=True, keep_ws=False):
    """One forward (with the final state) and one backward through ops; everything back on the CPU in the reference's layout.  keep_ws: the
    backward gets the forward's private workspace (kstate_valid)."""
    ops = _ops()
    B, T, H, dh = q.shape
    HD = H * dh
    qkv, g, omd = _dev(c, q, k, v, dout, om)
    qq, kk, vv = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    out, den, S, z = ops.favor_attn_fwd(qq, kk, vv, omd, B, T, H, eps=c['eps'], want_state=True)
    res = dict(out=out.view(B, T, H, dh), den=den, S=S, z=z)
    ws = None
    if keep_ws:
        out1, den1, ws = ops.favor_attn_fwd(qq, kk, vv, omd, B, T, H, eps=c['eps'], keep_ws=True)
        assert ws is not None and torch.equal(out1, out) and torch.equal(den1, den)
    if backward:
        if c['dn']:
            assert ops.favor_bwd_dn_ok(_dt(c), B, T, H, dh, c['nf'])
            g = dn_of(g.view(B, T, H, dh), den).view(B * T, HD).contiguous()
        grads = ops.favor_attn_bwd(qq, kk, vv, omd, out, g, None if c['dn'] else den, B, T, H, eps=c['eps'], ws_saved=ws, dn=c['dn'])
        res.update({n: t.reshape(B, T, H, dh) for n, t in zip(('dq', 'dk', 'dv'), grads)})
    torch.cuda.synchronize()
    return {n: t.detach().cpu().clone() for n, t in res.items()}


WORST = {}


def check(c, res, bd, names=('out', 'den', 'S', 'z', 'dq', 'dk', 'dv')):
    bad = []
    for n in names:
        r = bd.ratio(n, res[n])
        fam = c['fam'] + ('' if c['fs_bwd'] else '>bf16') + ('-dn' if c['dn'] else '')
        WORST[(fam, n)] = max(WORST.get((fam, n), 0.0), r)
        print('%s %s: max err/bound = %.3f' % (key(c), n, r))
        if not r <= 1.0:
            bad.append('%s %.3f' % (n, r))
    assert not bad, '%s: err/bound > 1: %s' % (key(c), ', '.join(bad))


def run_and_check(c, mp, keep_ws=False):
    _env(mp, c)
    ins, bd = inputs_and_bounds(c)
    res = run(c, *ins, keep_ws=keep_ws)
    if c['dn']:                                                    # dN is formed from the KERNEL's den, as in training: the reference takes the same dN
        bd = bounds_of(c, *ins, den_for_dn=res['den'].double())
    check(c, res, bd)
    return res


def teardown_module(module):
    for (fam, n), r in sorted(WORST.items()):
        print('worst err/bound  %-10s %-4s %.3f' % (fam, n, r))


# ---------------------------------------------------------------------------------------------------- (a) chunk edges, generic kernels
@pytest.mark.parametrize('fam,dh,nf', list(CASES_A))
def test_values_at_the_chunk_edges(fam, dh, nf, monkeypatch):
    for c in CASES_A[(fam, dh, nf)]:
        run_and_check(c, monkeypatch)


# ---------------------------------------------------------------------------------------------------- (b) segment edges
@pytest.mark.parametrize('c', CASES_B + [c for c in CASES_C if c['segs'] > 1], ids=key)
def test_values_at_the_segment_edges(c, monkeypatch):
    """Exact cut (256 = 2 x 128), a last segment whose last chunk is one token (257 = 192 + 64 + 1), a last segment shorter than a chunk
    (400 = 192 + 192 + 16), a request the geometry cuts down (16 wanted at T = 300: 2).  Backward with the state-only pass recomputed and with the
    forward's workspace kept (kstate_valid): same bits, both under the bound."""
    _env(monkeypatch, c)
    want = {(T, s): n for T, s, n in SEGMENTED}.get((c['T'], c['segs']), 2)
    assert _n_segments(c) == want == seg_len(c['T'], c['segs'])[0]
    a = run_and_check(c, monkeypatch)
    b = run_and_check(c, monkeypatch, keep_ws=True)
    for n in a:
        assert torch.equal(a[n], b[n]), '%s differs between the recomputed and the kept K-state increments' % n


# ---------------------------------------------------------------------------------------------------- (c) slice kernels
@pytest.mark.parametrize('c', [c for c in CASES_C if c['segs'] == 1], ids=key)
def test_slice_kernels_at_the_chunk_edges(c, monkeypatch):
    run_and_check(c, monkeypatch)


def test_slice_kernels_refuse_a_length_off_their_chunk_grid(monkeypatch):
    c = case('fs', 48)
    _env(monkeypatch, c)
    from emo_disentanger_amd._lib import EmoError
    ins = make_inputs(c)
    with pytest.raises(EmoError):
        run(c, *ins, backward=False)


# ---------------------------------------------------------------------------------------------------- (d) eps that matters, (e) loud tokens
@pytest.mark.parametrize('c', CASES_D, ids=key)
def test_eps_that_matters(c, monkeypatch):
    run_and_check(c, monkeypatch)


@pytest.mark.parametrize('c', CASES_E, ids=key)
def test_loud_tokens(c, monkeypatch):
    res = run_and_check(c, monkeypatch)
    for n, t in res.items():
        assert bool(torch.isfinite(t.float()).all()), n
    assert float(res['den'][:, :, 0].max()) <= 2 * c['eps'], 'den of the first token should have fallen to eps'


# ---------------------------------------------------------------------------------------------------- (f) causality
def _causal_cases():
    out = []
    for fam, T, segs in (('f32', 129, 1), ('bf16', 129, 1), ('fs', 96, 1), ('f32', 257, 2), ('bf16', 257, 2), ('fs', 256, 2)):
        C = max(chunks(fam, 64))
        t0s = [C - 1, C, C + 1] + ([seg_len(T, segs)[1]] if segs > 1 else [])
        out += [(case(fam, T, segs=segs), t0) for t0 in t0s]
    return out


@pytest.mark.parametrize('c,t0', _causal_cases(), ids=lambda x: key(x) if isinstance(x, dict) else str(x))
def test_causality_bit_for_bit(c, t0, monkeypatch):
    _env(monkeypatch, c)
    q, k, v, dout, om = make_inputs(c)
    q2, k2, v2, dout2, _ = make_inputs(c, seed=1)
    base = run(c, q, k, v, dout, om)
    fut = [torch.cat([a[:, :t0], b[:, t0:]], 1) for a, b in ((q, q2), (k, k2), (v, v2), (dout, dout2))]
    r1 = run(c, *fut, om)
    for n in ('out', 'dq'):
        assert torch.equal(base[n][:, :t0], r1[n][:, :t0]), '%s[:t0] changed with the future' % n
    assert torch.equal(base['den'][:, :, :t0], r1['den'][:, :, :t0])
    assert not torch.equal(base['out'][:, t0:], r1['out'][:, t0:])
    r2 = run(c, q, k, v, torch.cat([dout2[:, :t0], dout[:, t0:]], 1), om)
    for n in ('dk', 'dv'):
        assert torch.equal(base[n][:, t0:], r2[n][:, t0:]), '%s[t0:] changed with the past gradient' % n
    assert not torch.equal(base['dv'][:, :t0], r2['dv'][:, :t0])


# ---------------------------------------------------------------------------------------------------- (g) guards
def _sentinel(t):
    t.view(torch.int32 if t.element_size() == 4 else torch.int16).fill_(0x4B3C2D1E if t.element_size() == 4 else 0x4B3C)
    return t


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize('c', [case('f32', 17), case('f32', 65), case('bf16', 17), case('bf16', 65), case('fs', 96),
                               case('f32', 257, segs=2), case('bf16', 257, segs=2)], ids=key)
def test_nothing_outside_the_problem_is_read_or_written(c, monkeypatch):
    """q/k/v sit in a buffer with NaN rows behind row B*T and NaN columns beside the 3 H dh used ones; out, dout, dq, dk, dv have wider rows too,
    NaN beside dout; every output buffer is prefilled with a bit pattern, den / S / z with margins on both sides.  (All inside allocations.)"""
    from emo_disentanger_amd import _lib
    _env(monkeypatch, c)
    ins, bd = inputs_and_bounds(c)
    q, k, v, dout, om = ins
    B, T, H, dh = q.shape
    HD, F, dt, GR, GC, MG = H * dh, c['nf'], _dt(c), 70, 8, 64
    nan = float('nan')
    qkv = torch.full((B * T + GR, 3 * HD + GC), nan, dtype=dt, device='cuda')
    qkv[:B * T, :3 * HD] = torch.cat([t.reshape(B * T, HD) for t in (q, k, v)], 1).to(dt)
    g = torch.full((B * T + GR, HD + GC), nan, dtype=dt, device='cuda')
    g[:B * T, :HD] = dout.reshape(B * T, HD).to(dt)
    out = _sentinel(torch.empty(B * T + GR, HD + GC, dtype=dt, device='cuda'))
    dqkv = _sentinel(torch.empty(B * T + GR, 3 * HD + GC, dtype=dt, device='cuda'))
    den, S, z = [_sentinel(torch.empty(n + 2 * MG, dtype=torch.float32, device='cuda')) for n in (B * H * T, B * H * F * dh, B * H * F)]
    omd = om.cuda()
    wsb = _lib.lib.emo_favor_attn_workspace_bytes(B, T, H, dh, F)
    ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device='cuda')
    p, es = _lib.ptr, qkv.element_size()
    common = dict(kind=_lib.ATTN_FAVOR, q=p(qkv), k=qkv.data_ptr() + HD * es, v=qkv.data_ptr() + 2 * HD * es, ld=3 * HD + GC, out=p(out), ld_out=HD + GC,
                  dtype=_lib.dtype_code(dt), B=B, T=T, H=H, dh=dh, omega=p(omd), den=den.data_ptr() + 4 * MG, n_feat=F, eps=c['eps'],
                  workspace=p(ws) if wsb else None, workspace_bytes=wsb)
    a = _lib.Attn(pass_=_lib.ATTN_FWD, state_S=S.data_ptr() + 4 * MG, state_z=z.data_ptr() + 4 * MG, **common)
    _lib.check(_lib.lib.emo_attn(ctypes.byref(a), _lib.stream()))
    a = _lib.Attn(pass_=_lib.ATTN_BWD, dout=p(g), dq=p(dqkv), dk=dqkv.data_ptr() + HD * es, dv=dqkv.data_ptr() + 2 * HD * es, ld_d=3 * HD + GC, **common)
    _lib.check(_lib.lib.emo_attn(ctypes.byref(a), _lib.stream()))
    torch.cuda.synchronize()
    res = dict(out=out[:B * T, :HD].reshape(B, T, H, dh), den=den[MG:-MG].view(B, H, T), S=S[MG:-MG].view(B, H, F, dh), z=z[MG:-MG].view(B, H, F))
    res.update({n: dqkv[:B * T, i * HD:(i + 1) * HD].reshape(B, T, H, dh) for i, n in enumerate(('dq', 'dk', 'dv'))})
    check(c, {n: t.cpu() for n, t in res.items()}, bd)
    for name, buf, cols in (('out', out, HD), ('dq/dk/dv', dqkv, 3 * HD)):
        ref = _sentinel(torch.empty_like(buf))
        assert torch.equal(_bits(buf)[B * T:], _bits(ref)[B * T:]), name + ': rows behind B*T were written'
        assert torch.equal(_bits(buf)[:, cols:], _bits(ref)[:, cols:]), name + ': columns beside the problem were written'
    for name, buf in (('den', den), ('S', S), ('z', z)):
        ref = _sentinel(torch.empty_like(buf))
        assert torch.equal(_bits(buf)[:MG], _bits(ref)[:MG]) and torch.equal(_bits(buf)[-MG:], _bits(ref)[-MG:]), name + ': written outside its extent'


# ---------------------------------------------------------------------------------------------------- (h) streams and heads
@pytest.mark.parametrize('c', [case('f32', 65), case('bf16', 65), case('f32', 33, 16, 32), case('bf16', 33, 16, 32), case('fs', 96),
                               case('f32', 257, segs=2), case('bf16', 257, segs=2), case('fs', 256, segs=2)], ids=key)
def test_streams_and_heads_do_not_mix(c, monkeypatch):
    _env(monkeypatch, c)
    q, k, v, dout, om = make_inputs(c)
    base = run(c, q, k, v, dout, om)
    again = run(c, q, k, v, dout, om)
    for n in base:
        assert torch.equal(base[n], again[n]), '%s: two identical calls differ' % n
    sw = run(c, *[t.flip(0) for t in (q, k, v, dout)], om)
    for n in base:
        assert torch.equal(base[n].flip(0), sw[n]), '%s: swapping the streams does not swap the result' % n
    for h in range(c['H']):
        one = run(dict(c, H=1), *[t[:, :, h:h + 1].contiguous() for t in (q, k, v, dout)], om)
        for n in base:
            sel = base[n][:, h:h + 1] if n in ('den', 'S', 'z') else base[n][:, :, h:h + 1]
            assert torch.equal(sel, one[n]), '%s: head %d alone (H = 1) differs from its columns in the H = %d call' % (n, h, c['H'])
