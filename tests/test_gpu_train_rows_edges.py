"""The training row kernels (csrc/emo_elementwise.hip, the logits-row kernels in csrc/emo_score.hip, colsum in csrc/emo_gemm.hip) at the edges of their ranges, against float64 references
computed on the CPU from the same stored inputs (bf16 values upcast exactly, so both sides start from identical numbers).

Covered here and nowhere else: the LayerNorm template selection at D = 4 / 260 / 512 / 768 (NV = 4 with a dead fourth group) / 1024, rows with a
large mean and constant rows, every argument combination of the backward (dres / dx_drop / dcol present or not), the grid-stride loops behind the
block caps, the 16-byte alignment fallback; per-row lse of the cross-entropy at the dispatch edges (M >= 1024, V <= 384, V <= 512), shifted rows,
-inf entries, an all-ignored batch; argmax ties and all -inf rows; sumsq / clip_coef / adam_step at n = 1 and past their block caps, without
gscale / without the bf16 mirror, at a large step, with `denom`; emo_cast; colsum's scalar fallbacks, row tails, several column blocks, accumulate.

Every tolerance is a bound derived from the kernel's arithmetic with u = 2^-24 (fp32 unit round-off), written where it is used; each assertion
prints max err / tol.  NaN logits are out of scope: the kernels' NaN rule (first NaN of a lane wins) is not pinned here.

Observed max err / tol on the MI355X (the worst case of each family over all parametrisations):
    LayerNorm forward   mean 0.036, rstd 0.154, y 0.367 (fp32) / 0.996 (bf16)
    LayerNorm backward  dx 0.154 (fp32) / 0.996 (bf16), dgamma 0.29, dbeta 0.000, dcol 0.099
    cross-entropy       lse 0.092 (xent_fwd and token_scores), acc[0] 0.035, gradient 0.238 (fp32) / 0.995 (bf16)
    sumsq 0.013, clip_coef 0.283, adam m 0.406, v 0.668, p 1.000, colsum 0.001
The ratios at 0.99 .. 1.00 are the output rounding itself: the bf16 bounds' last term is half a bf16 ulp of the result and adam's first term half an
fp32 ulp of p, which round-to-nearest reaches; the arithmetic terms in front of them are used to a third at most.  The column sums (dbeta, colsum)
are almost exact because sums of a few thousand bf16-representable values fit the fp32 mantissa."""
import math

import numpy as np
import pytest
import torch

import dropmask_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DT = [torch.float32, torch.bfloat16]
EPS = float(np.float32(1e-5))
INF = float('inf')


def _ops():
    from emo_disentanger_amd import ops
    return ops


def _out_round(dt):
    return 2.0 ** -23 if dt == torch.float32 else 2.0 ** -8


def _dn(dt):
    return 'f32' if dt == torch.float32 else 'bf16'


def _bf(*shape, seed=0, scale=1.0, shift=0.0):
    """fp32 tensor of bf16-representable values"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(torch.bfloat16).float()


def _ratio(err, tol):
    """max err / tol (0 / 0 counts as 0)"""
    err, tol = err.double().reshape(-1), tol.double().reshape(-1).expand(err.numel())
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(r.max()) if r.numel() else 0.0


def _check(name, got, ref, tol):
    assert bool(torch.isfinite(got.double()).all()), '%s: non-finite values' % name
    r = _ratio((got.double().cpu() - ref.double()).abs(), tol if torch.is_tensor(tol) else torch.tensor(float(tol)))
    print('%s: max err/tol = %.3f' % (name, r))
    assert r <= 1.0, '%s: max err/tol = %.3f' % (name, r)
    return r


# ==================================================================================================== LayerNorm
def _ln_rows(M, D, seed):
    """Row families by row index mod 5: 0, 1: N(0, 1); 2, 3: mean = 100 std; 4: constant (3.0: every partial sum of the row is exact in fp32)."""
    x = _bf(M, D, seed=seed)
    for i in range(M):
        if i % 5 in (2, 3):
            x[i] = (x[i] + 100.0).to(torch.bfloat16).float()
        elif i % 5 == 4:
            x[i] = 3.0
    return x


def _ln_fwd_check(tag, dt, x, gm, bt, y, mean, rstd):
    """x: the stored input (fp32 view of it); y, mean, rstd: the kernel's.  float64 reference and the derived bounds."""
    M, D = x.shape
    L = math.log2(D)
    xd, g, b = x.double(), gm.double(), bt.double()
    mu = xd.mean(1)
    d = xd - mu[:, None]
    var = (d * d).mean(1)
    rs = 1.0 / torch.sqrt(var + EPS)
    # mean: a sum of D terms (<= 16 in a lane, 6 shuffle levels) and one division
    tol_mu = (L + 4) * U * xd.abs().mean(1)
    _check(tag + ' mean', mean, mu, tol_mu)
    # rstd = (var + eps)^-1/2, var = mean((x - mean^)^2): a deviation carries the mean's error and one rounding, |d^ - d| <= tol_mu + u |d|, so
    # |var^ - var| <= 2 mean|d| tol_mu + tol_mu^2 + 3 u var (squares) + (log2 D + 4) u var (the sum, as for the mean); the relative error of
    # rstd is half that over var + eps, plus the add of eps (u) and rsqrtf (<= 2 ulp = 4 u with the final rounding)
    dvar = 2 * d.abs().mean(1) * tol_mu + tol_mu ** 2 + (L + 7) * U * var
    tol_rs = rs * (0.5 * dvar / (var + EPS) + 5 * U)
    _check(tag + ' rstd', rstd, rs, tol_rs)
    yref = d * rs[:, None] * g + b
    tol_y = rs[:, None] * g.abs() * (L + 8) * U * (mu.abs()[:, None] + d.abs()) + _out_round(dt) * yref.abs()
    _check(tag + ' y', y, yref, tol_y)
    const = [i for i in range(M) if i % 5 == 4]
    if const:                                              # constant rows: rstd = 1 / sqrt(eps) to fp32 rounding, y = beta (rounded to the storage type)
        assert bool(((rstd.double().cpu()[const] - EPS ** -0.5).abs() <= 5 * U * EPS ** -0.5).all())
        assert torch.equal(y.cpu()[const], bt.to(dt).expand(len(const), D)), tag + ': y of a constant row is not beta'


def _ln_bwd_ref(x, dy, gm, mean, rstd, dres):
    """float64 dx / dgamma terms / dbeta terms from the stored inputs (mean and rstd are INPUTS of the backward)."""
    xd, a, g, mu, rs = x.double(), dy.double(), gm.double(), mean.double().cpu()[:, None], rstd.double().cpu()[:, None]
    xh = (xd - mu) * rs
    gy = a * g
    s1, s2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    dx = rs * (gy - s1 - xh * s2) + (dres.double() if dres is not None else 0.0)
    # the same pattern as y: every term of rstd (gy - mean(gy) - xh mean(gy xh)) carries (log2 D + 8) u of its own magnitude (sums by their
    # absolute terms), the result is rounded once to the storage type
    mag = gy.abs() + gy.abs().mean(1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(1, keepdim=True)
    return dx, rs * mag, a * xh, a


def _ln_bwd_check(tag, dt, x, dy, dres, gm, mean, rstd, p=0.25, seed=(5 << 32) | 9, offset=4107, combos=('full', 'nodres', 'nodrop', 'nodcol')):
    """x, dy, dres: fp32 CPU tensors of values representable in dt; runs the backward in each argument combination."""
    ops = _ops()
    M, D = x.shape
    L = math.log2(D)
    xg, dyg, drg, gmg = x.to(dt).cuda(), dy.to(dt).cuda(), dres.to(dt).cuda(), gm.cuda()
    worst = {}
    for combo in combos:
        dr = None if combo == 'nodres' else dres
        want_drop = combo != 'nodrop'
        dg, db = torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')
        dcol = None if combo == 'nodcol' else torch.zeros(D, device='cuda')
        dx, dxd = ops.layernorm_bwd(dyg, xg, gmg, mean, rstd, dg, db, dres=None if dr is None else drg, want_drop=want_drop, p_drop=p, seed=seed,
                                    offset=offset, dcol=dcol)
        ref, mag, tg, tb = _ln_bwd_ref(x, dy, gm, mean, rstd, dr)
        t = '%s %s' % (tag, combo)
        worst['dx'] = max(worst.get('dx', 0), _check(t + ' dx', dx, ref, (L + 8) * U * mag + _out_round(dt) * ref.abs()))
        # column sums: fp32 summation of M terms as a random walk with an 8 x margin, 8 sqrt(M) u sum|term| (the worst case is M u sum|term|)
        cs = 8 * math.sqrt(M) * U
        worst['dgamma'] = max(worst.get('dgamma', 0), _check(t + ' dgamma', dg, tg.sum(0), cs * tg.abs().sum(0)))
        worst['dbeta'] = max(worst.get('dbeta', 0), _check(t + ' dbeta', db, tb.sum(0), cs * tb.abs().sum(0)))
        dxc = dx.double().cpu()
        if want_drop:                                      # the consumer re-reads dx in storage precision: the mask applies to the ROUNDED value
            mult = torch.from_numpy(R.multipliers((M, D), p, seed, offset))
            assert torch.equal(dxd.float().cpu(), (dx.float().cpu() * mult).to(dt).float()), t + ': dx_drop is not round(dx) * port multiplier'
            dxc = dxd.double().cpu()
        else:
            assert dxd is None
        if dcol is not None:                               # column sum of the rounded dx (dx_drop when it is written), as the kernel states
            worst['dcol'] = max(worst.get('dcol', 0), _check(t + ' dcol', dcol, dxc.sum(0), cs * dxc.abs().sum(0)))
    return worst


@pytest.mark.parametrize('dt', DT, ids=['f32', 'bf16'])
@pytest.mark.parametrize('M', [1, 5])
@pytest.mark.parametrize('D', [4, 260, 512, 768, 1024])
def test_layernorm_template_edges_row_families_and_argument_combinations(D, M, dt):
    """D = 4 (one live lane), 260 (NV = 2, one live lane in the second group), 512, 768 (nv == 3 on the NV = 4 instance), 1024; N(0, 1), large-mean
    and constant rows."""
    ops = _ops()
    x = _ln_rows(M, D, seed=D + M)
    gm, bt = _bf(D, seed=2) * 0.1 + 1, _bf(D, seed=3)
    y, mean, rstd = ops.layernorm_fwd(x.to(dt).cuda(), gm.cuda(), bt.cuda(), eps=1e-5)
    _ln_fwd_check('ln %s D=%d M=%d' % (_dn(dt), D, M), dt, x, gm, bt, y, mean, rstd)
    _ln_bwd_check('ln_bwd %s D=%d M=%d' % (_dn(dt), D, M), dt, x, _bf(M, D, seed=4), _bf(M, D, seed=5), gm, mean, rstd)


@pytest.mark.parametrize('dt, M, D', [(torch.float32, 4099, 64), (torch.bfloat16, 4099, 64), (torch.bfloat16, 4101, 512)], ids=['f32-64', 'bf16-64', 'bf16-512'])
def test_layernorm_many_rows_against_float64(dt, M, D):
    """M = 4099 at D = 64: 1025 row quads on the backward's 1024-block cap, so waves loop; M = 4101 at D = 512 bf16: the 16-byte kernels (forward
    from M = 4096), their odd row tail, and dgamma / dbeta / dcol of the workspace variant against float64, not against the atomic variant."""
    ops = _ops()
    x = _ln_rows(M, D, seed=11)
    gm, bt = _bf(D, seed=2) * 0.1 + 1, _bf(D, seed=3)
    y, mean, rstd = ops.layernorm_fwd(x.to(dt).cuda(), gm.cuda(), bt.cuda(), eps=1e-5)
    _ln_fwd_check('ln %s D=%d M=%d' % (_dn(dt), D, M), dt, x, gm, bt, y, mean, rstd)
    _ln_bwd_check('ln_bwd %s D=%d M=%d' % (_dn(dt), D, M), dt, x, _bf(M, D, seed=4), _bf(M, D, seed=5), gm, mean, rstd)


def _view4(t):
    """the same values as a contiguous view 4 elements into a larger buffer (fp32: still 16-byte aligned; bf16: 8 bytes off)"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize('dt, M, D', [(torch.float32, 37, 512), (torch.float32, 37, 260), (torch.bfloat16, 4101, 512), (torch.bfloat16, 37, 260)],
                         ids=['f32-512', 'f32-260', 'bf16-512', 'bf16-260'])
def test_layernorm_inputs_at_an_offset_of_four_elements(dt, M, D):
    """x and dy as views 4 elements into a larger buffer.  The generic kernels do not care (bit-equal results); the bf16 D = 512 kernels need 16-byte
    alignment and hand the call to the generic ones: results within the same float64 bounds."""
    ops = _ops()
    x, dy, dres = _ln_rows(M, D, seed=21), _bf(M, D, seed=4), _bf(M, D, seed=5)
    gm, bt = (_bf(D, seed=2) * 0.1 + 1).cuda(), _bf(D, seed=3).cuda()
    xa, dya, drg = x.to(dt).cuda(), dy.to(dt).cuda(), dres.to(dt).cuda()
    xv, dyv = _view4(xa), _view4(dya)
    assert xv.data_ptr() % 16 == (0 if dt == torch.float32 else 8) and xv.is_contiguous()
    ya, ma, ra = ops.layernorm_fwd(xa, gm, bt)
    yv, mv, rv = ops.layernorm_fwd(xv, gm, bt)
    outs = []
    for xi, dyi, mi, ri in ((xa, dya, ma, ra), (xv, dyv, mv, rv)):
        dg, db, dcol = torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda'), torch.zeros(D, device='cuda')
        dx, dxd = ops.layernorm_bwd(dyi, xi, gm, mi, ri, dg, db, dres=drg, want_drop=True, p_drop=0.25, seed=9, offset=2, dcol=dcol)
        outs.append((dx, dxd))
    if not (dt == torch.bfloat16 and D == 512):
        assert torch.equal(ya, yv) and torch.equal(ma, mv) and torch.equal(ra, rv)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    else:
        _ln_fwd_check('ln view', dt, x, gm.cpu(), bt.cpu(), yv, mv, rv)
        ref, mag, _, _ = _ln_bwd_ref(x, dy, gm.cpu(), mv, rv, dres)
        _check('ln_bwd view dx', outs[1][0], ref, (math.log2(D) + 8) * U * mag + _out_round(dt) * ref.abs())


# ==================================================================================================== cross-entropy
MS, VS = [1023, 1024, 1025], [63, 64, 65, 384, 385, 512, 513]


def _xent_case(M, V, seed):
    """logits 3 N(0, 1) (bf16 values); rows i % 4 == 1 shifted by +100, == 2 by -100 (expf over- / underflows without the max subtraction),
    == 3 with a quarter of the entries -inf, never the target column."""
    g = torch.Generator().manual_seed(seed)
    l = _bf(M, V, seed=seed, scale=3.0)
    tgt = torch.randint(0, V, (M,), generator=g)
    l[1::4] = (l[1::4] + 100.0).to(torch.bfloat16).float()
    l[2::4] = (l[2::4] - 100.0).to(torch.bfloat16).float()
    hole = torch.rand(M, V, generator=g) < 0.25
    hole[torch.arange(M), tgt] = False
    hole[torch.arange(M) % 4 != 3] = False
    l[hole] = -INF
    return l, tgt


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('M', MS)
def test_xent_rows_at_the_dispatch_edges(M, V):
    """M >= 1024 selects the two-rows-per-wave register kernels (V <= 384: NV = 6, V <= 512: NV = 8), M = 1025 their odd tail; below / above, the
    generic kernel.  Per-row lse, the loss sum and count, the gradient and its padding columns against float64."""
    ops = _ops()
    l, tgt0 = _xent_case(M, V, seed=M + V)
    ld = l.double()
    lse_ref = torch.logsumexp(ld, 1)
    # lse = max + logf(sum expf(l - max)): a sum of V terms in [0, 1] of which one is 1 (log2 V levels and the lane's serial part), expf and logf
    # of a few ulp each, two roundings
    tol_lse = (math.log2(V) + 8) * U * lse_ref.abs().clamp(min=1.0)
    lg = l.cuda()
    for ignore in (-100, 5):                               # outside and inside the vocabulary
        tgt = tgt0.clone()
        if ignore == -100:
            tgt[::7] = -100
        valid = tgt != ignore
        lse, acc = ops.xent_fwd(lg, tgt.cuda(), ignore)
        _check('xent M=%d V=%d lse' % (M, V), lse, lse_ref, tol_lse)
        ts = ops.token_scores(lg, tgt.cuda(), ignore, want=('lse',))
        _check('token_scores M=%d V=%d lse' % (M, V), ts['lse'], lse_ref, tol_lse)
        loss = (lse_ref - ld.gather(1, tgt.clamp(min=0)[:, None])[:, 0])[valid]
        acc = acc.double().cpu()
        assert float(acc[1]) == float(valid.sum()), (float(acc[1]), int(valid.sum()))
        # per-row terms within the lse bound (a 1 / sqrt(M) share of the budget at most), then fp32 summation of M terms as a random walk
        r = abs(float(acc[0]) - float(loss.sum())) / (8 * math.sqrt(M) * U * float(loss.abs().sum()))
        print('xent M=%d V=%d acc[0]: err/tol = %.3f' % (M, V, r))
        assert r <= 1.0, 'acc[0]: err/tol = %.3f' % r
        for odt in DT:
            gs = torch.tensor([0.37], device='cuda')
            ldo = (V + 7) // 8 * 8 + 8
            dl = ops.xent_bwd(lg, tgt.cuda(), lse, gs, ignore, odt, ld_out=ldo)
            assert dl.shape == (M, ldo) and bool((dl[:, V:] == 0).all()), 'padding columns are not zero'
            gsf = float(gs.float().cpu())
            onehot = torch.zeros(M, V, dtype=torch.float64)
            onehot[torch.arange(M)[valid], tgt[valid]] = 1.0
            gref = (torch.exp(ld - lse.double().cpu()[:, None]) - onehot) * gsf * valid[:, None].double()
            _check('xent_bwd M=%d V=%d %s' % (M, V, _dn(odt)), dl[:, :V], gref, 4 * U * gsf + _out_round(odt) * gref.abs())


@pytest.mark.parametrize('M, V', [(1023, 65), (1025, 384), (1025, 513)])
def test_xent_all_ignored_batch(M, V):
    ops = _ops()
    l, _ = _xent_case(M, V, seed=3)
    for ignore in (-100, 7):
        tgt = torch.full((M,), ignore, dtype=torch.int64).cuda()
        lse, acc = ops.xent_fwd(l.cuda(), tgt, ignore)
        assert acc.cpu().tolist() == [0.0, 0.0]
        for odt in DT:
            dl = ops.xent_bwd(l.cuda(), tgt, lse, torch.ones(1, device='cuda'), ignore, odt)
            assert bool((dl == 0).all())


# ==================================================================================================== argmax / accuracy counts
def _argmax_case(M, V, seed):
    """Random rows with exact ties planted (block of 8 rows, repeated at the start, in the middle and at the very end so that both rows of a
    two-row step and the odd tail are hit): 0: two lanes; 1: one lane, columns c and c + 64; 2: first and last column; 3: maximum at V - 1;
    4: all -inf; 5: tie of three; 6: all equal; 7: -inf except the last column."""
    l = _bf(M, V, seed=seed, scale=3.0)
    for base in (0, 9, M // 2, M - 8):
        top = 64.0
        r = l[base:base + 8]
        r[0, [3, 41]] = top
        if V > 64:
            r[1, [V - 65, V - 1]] = top
        r[2, [0, V - 1]] = top
        r[3, V - 1] = top
        r[4, :] = -INF
        r[5, [V - 1, 17, 30]] = top
        r[6, :] = 1.5
        r[7, :] = -INF
        r[7, V - 1] = -1e30
    return l


@pytest.mark.parametrize('V', VS)
@pytest.mark.parametrize('M', MS)
def test_argmax_and_accuracy_counts_ties_and_all_minus_inf_rows(M, V):
    """The lowest index among equal maxima, as numpy.argmax; index 0 for a row of -inf only (the kernels returned INT64_MAX: nothing beats the start
    value -inf).  accuracy_counts runs the generic kernel (M < 1024 or V > 512) and both register kernels."""
    ops = _ops()
    l = _argmax_case(M, V, seed=M * 7 + V)
    ref = torch.from_numpy(np.argmax(l.numpy(), axis=1))
    assert int(ref[4]) == 0 and int(ref[M - 4]) == 0 and int(ref[3]) == V - 1 and int(ref[2]) == 0
    got = ops.argmax(l.cuda()).cpu()
    bad = (got != ref).nonzero().view(-1)
    assert bad.numel() == 0, 'rows %s: got %s, numpy %s' % (bad[:8].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())
    g = torch.Generator().manual_seed(1)
    tgt = torch.where(torch.rand(M, generator=g) < 0.7, ref, torch.randint(0, V, (M,), generator=g))      # the planted rows mostly count as hits
    pad = 2
    chord, melody = (torch.rand(M, generator=g) < 0.3).long(), (torch.rand(M, generator=g) < 0.5).long()
    ok = ref == tgt
    exp = [int((tgt != pad).sum()), int((ok & (tgt != pad)).sum()), int(chord.sum()), int((ok & (chord == 1)).sum()), int(melody.sum()),
           int((ok & (melody == 1)).sum())]
    assert ops.accuracy_counts(l.cuda(), tgt.cuda(), chord.cuda(), melody.cuda(), pad).cpu().tolist() == exp
    # an all -inf batch with target 0 everywhere: every row is a hit
    ninf = torch.full((M, V), -INF).cuda()
    assert ops.argmax(ninf).cpu().tolist() == [0] * M
    assert ops.accuracy_counts(ninf, torch.zeros(M, dtype=torch.int64).cuda(), None, None, pad).cpu().tolist() == [M, M, 0, 0, 0, 0]


# ==================================================================================================== sumsq / clip_coef / adam_step
@pytest.mark.parametrize('n', [1, 3, 5, 1024 * 256 * 4 + 5])
def test_sumsq_tails_and_past_the_block_cap(n):
    """n = 1, 3: only the scalar tail of thread 0; 5: one vector and a tail; 1024 x 256 x 4 + 5: one vector more than the capped grid covers in one
    pass (thread 0 loops), plus the tail.  All terms are positive: <= ceil(n / 2^20) + 3 adds per thread, 6 shuffle levels and 3 adds,
    twice (blocks, then the partials) — under 40 roundings, so 64 u relative."""
    ops = _ops()
    x = _bf(n, seed=n % 97)
    ss = torch.zeros(ops.SUMSQ_FLOATS, device='cuda')
    ops.sumsq(x.cuda(), ss)
    first = ss[0].clone()
    ops.sumsq(x.cuda(), ss)                                 # scratch reusable without re-zeroing; fixed summation order => the same bits
    assert torch.equal(first, ss[0]) and int(ss[1025].view(torch.int32)) == 0
    ref = float((x.double() ** 2).sum())
    r = abs(float(first) - ref) / (64 * U * ref)
    print('sumsq n=%d: err/tol = %.3f' % (n, r))
    assert r <= 1.0, 'sumsq n=%d: err/tol = %.3f' % (n, r)


def _clip_ref(ss, max_norm, pre, denom):
    f = lambda v: float(np.float32(v))
    pre = f(pre)
    if denom is not None:
        pre = pre / denom if denom > 0 else 0.0
    total = math.sqrt(ss) * pre
    c = f(max_norm) / (total + f(1e-6))
    return min(c, 1.0) * pre


@pytest.mark.parametrize('ss, max_norm, pre, denom', [(0.04, 0.5, 1.0 / 3, None), (7.3, 0.5, 1.0 / 3, None), (900.0, 0.5, 0.75, None),
                                                      (7.3, 0.5, 1.0, 37.0), (1e6, 0.5, 1.0, 1999.0), (7.3, 0.5, 1.0, 0.0)])
def test_clip_coef_against_the_float64_formula(ss, max_norm, pre, denom):
    """Below and above max_norm with pre != 1; the token-weighted data-parallel form pre / denom (optim.py), denom == 0 -> exactly 0."""
    ops = _ops()
    sst = torch.zeros(ops.SUMSQ_FLOATS, device='cuda')
    sst[0] = ss
    coef = torch.full((1,), -1.0, device='cuda')
    dn = None if denom is None else torch.tensor([denom], device='cuda')
    ops.clip_coef(sst, max_norm, pre, coef, denom=dn)
    got = float(coef.cpu())
    ref = _clip_ref(float(sst[0].cpu()), max_norm, pre, denom)
    if denom == 0.0:
        assert got == 0.0
        return
    r = abs(got - ref) / (4 * U * abs(ref))
    print('clip_coef: err/tol = %.3f' % r)
    assert r <= 1.0, 'clip_coef %s: got %.9g ref %.9g err/tol = %.3f' % ((ss, max_norm, pre, denom), got, ref, r)


@pytest.mark.parametrize('mirror, scaled', [(True, True), (False, True), (True, False)], ids=['mirror+gscale', 'no-mirror', 'no-gscale'])
@pytest.mark.parametrize('step', [1, 10, 100000])
@pytest.mark.parametrize('n', [1, 4096 * 256 + 3])
def test_adam_one_step_from_nonzero_moments(n, step, mirror, scaled):
    """One step from non-zero m and v against float64.  g and m share their sign, so m' = m + (g - m)(1 - b1) does not cancel and the bounds are
    relative to the new moments: |dm| <= 4 u |m'| (g gs, the difference, the product, the sum), |dv| <= 4 u |v'|; p' = p - (lr / bc1) m' /
    (sqrt(v') / sqrt(bc2) + eps): one rounding of p plus a chain of ~8 roundings (16 u) on the update."""
    ops = _ops()
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    f = lambda v: float(np.float32(v))
    sign = torch.where(_bf(n, seed=1) >= 0, 1.0, -1.0)
    g, m0 = (_bf(n, seed=2).abs() + 0.01) * sign, (_bf(n, seed=3).abs() * 0.5 + 0.01) * sign
    v0, p0 = (_bf(n, seed=4) ** 2) * 0.7 + 1e-4, _bf(n, seed=5)
    gs = f(0.37) if scaled else 1.0
    p, m, v = p0.clone().cuda(), m0.clone().cuda(), v0.clone().cuda()
    pb = torch.zeros(n, device='cuda', dtype=torch.bfloat16) if mirror else None
    ops.adam_step(p, g.cuda(), m, v, pb, lr, b1, b2, eps, step, torch.tensor([gs], device='cuda') if scaled else None)
    gi = g.double() * gs
    mr = m0.double() + (gi - m0.double()) * (1.0 - f(b1))
    vr = v0.double() * f(b2) + (1.0 - f(b2)) * gi * gi
    bc1, bc2 = 1.0 - f(b1) ** step, 1.0 - f(b2) ** step
    upd = f(lr) * (mr / bc1) / (torch.sqrt(vr / bc2) + f(eps))
    pr = p0.double() - upd
    tag = 'adam n=%d step=%d' % (n, step)
    _check(tag + ' m', m, mr, 4 * U * mr.abs())
    _check(tag + ' v', v, vr, 4 * U * vr.abs())
    _check(tag + ' p', p, pr, U * pr.abs() + 16 * U * upd.abs())
    if mirror:
        assert torch.equal(pb.view(torch.int16), p.to(torch.bfloat16).view(torch.int16))


# ==================================================================================================== cast
def _special_f32():
    bits = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,          # exact ties: to even down (1.00390625 -> 1.0), up (-> 1.015625), both signs
            0x3F808001, 0x3F807FFF,                                  # one ulp either side of a tie
            0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,          # largest finite -> inf; the tie below inf -> inf (even); just under -> largest bf16
            0x00000001, 0x007FFFFF, 0x80000001, 0x00008000, 0x00018000, 0x00400000,      # subnormals (bf16 keeps them: same exponent range)
            0x00000000, 0x80000000, 0x7F800000, 0xFF800000,          # +-0, +-inf
            0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]          # NaNs, one with payload only in the low 16 bits
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


@pytest.mark.parametrize('n', [1, 4096 * 256 + 3])
def test_cast_round_to_nearest_even_specials_and_past_the_block_cap(n):
    """fp32 -> bf16 equals torch's .to(bfloat16) bit for bit (NaN stays NaN), bf16 -> fp32 is exact, same-type casts are copies."""
    ops = _ops()
    g = torch.Generator().manual_seed(n % 89)
    x = torch.randn(n, generator=g) * torch.exp(4 * torch.randn(n, generator=g))
    sp = _special_f32()
    if n > sp.numel():
        x[:sp.numel()] = sp
        x[-3:] = sp[:3]
    for src in ([x] if n > 1 else [x] + [sp[i:i + 1].clone() for i in range(sp.numel())]):
        ref = src.to(torch.bfloat16)
        got = ops.cast(src.cuda(), torch.empty(src.numel(), device='cuda', dtype=torch.bfloat16)).cpu()
        nan = torch.isnan(ref)
        assert torch.equal(torch.isnan(got), nan)
        bad = (got.view(torch.int16) != ref.view(torch.int16)) & ~nan
        assert not bool(bad.any()), 'fp32 -> bf16: %d differ, first input bits %08x' % (int(bad.sum()), int(src.view(torch.int32)[bad][0]) & 0xFFFFFFFF)
        back = ops.cast(ref.cuda(), torch.empty(src.numel(), device='cuda', dtype=torch.float32)).cpu()
        assert torch.equal(back.view(torch.int32)[~nan], ref.float().view(torch.int32)[~nan]) and bool(torch.isnan(back[nan]).all())
        keep = ~torch.isnan(src)
        same = ops.cast(src.cuda(), torch.empty(src.numel(), device='cuda', dtype=torch.float32)).cpu()
        assert torch.equal(same.view(torch.int32)[keep], src.view(torch.int32)[keep])
        same16 = ops.cast(ref.cuda(), torch.empty(src.numel(), device='cuda', dtype=torch.bfloat16)).cpu()
        assert torch.equal(same16.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])


# ==================================================================================================== colsum
def _colsum_check(tag, X, Xcpu, accumulate=False):
    ops = _ops()
    M, N = Xcpu.shape
    out0 = _bf(N, seed=8) if accumulate else None
    out = out0.clone().cuda() if accumulate else torch.full((N,), float('nan'), device='cuda')
    got = ops.colsum(X, out=out, accumulate=accumulate)
    ref = Xcpu.double().sum(0) + (out0.double() if accumulate else 0.0)
    tol = 8 * math.sqrt(M) * U * (Xcpu.double().abs().sum(0) + (out0.double().abs() if accumulate else 0.0))
    return _check(tag, got, ref, tol)


@pytest.mark.parametrize('dt', DT, ids=['f32', 'bf16'])
@pytest.mark.parametrize('M, N', [(1, 8), (13, 136), (67, 520), (1030, 264)])
def test_colsum_shapes_tails_and_column_blocks(M, N, dt):
    """Row tails that are no multiple of 16 (the 4 x unrolled loop and its remainder), a last partial column group, more than one column block
    (N > 256 fp32 / > 512 bf16), more than one row split (M = 1030), accumulate into a non-zero vector."""
    x = _bf(M, N, seed=M + N)
    _colsum_check('colsum %s %dx%d' % (_dn(dt), M, N), x.to(dt).cuda(), x)
    _colsum_check('colsum %s %dx%d acc' % (_dn(dt), M, N), x.to(dt).cuda(), x, accumulate=True)


@pytest.mark.parametrize('dt, ld', [(torch.float32, 56), (torch.float32, 51), (torch.bfloat16, 56), (torch.bfloat16, 51)])
@pytest.mark.parametrize('M', [13, 67])
def test_colsum_scalar_fallbacks(M, dt, ld):
    """N = 50: the last column group is partial (scalar path); ld = 51: ld % VE != 0 sends every group down the scalar path; a view starting one
    element into its buffer: the pointer is not 16-byte aligned."""
    N = 50
    x = _bf(M, N, seed=M + ld)
    buf = torch.zeros(M * ld + 8, dtype=dt, device='cuda')
    for start in (0, 1):
        v = buf[start:start + M * ld].view(M, ld)[:, :N]
        v.copy_(x.to(dt))
        assert v.data_ptr() % 16 == (0 if start == 0 else (4 if dt == torch.float32 else 2))
        _colsum_check('colsum N=50 ld=%d start=%d' % (ld, start), v, x)
        _colsum_check('colsum N=50 ld=%d start=%d acc' % (ld, start), v, x, accumulate=True)
