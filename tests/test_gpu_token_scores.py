"""GPU kernel tests of the sequence-scoring entry points (emo_score.hip): ops.token_scores against a float64 restatement on the SAME fp32
logits, ops.xent_bwd_rows against torch autograd, and both against the training-path kernels they mirror (ops.xent_fwd / ops.xent_bwd /
ops.argmax)."""
import pytest
import torch

from test_gpu_train_rows_edges import MS as EDGE_MS, VS as EDGE_VS, _argmax_case, _xent_case

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
ROW_TOL = 1e-5          # absolute, per row: the bound test_xent_fwd_bwd_and_accuracy holds the mean loss to, at the same logit scale (randn x 3:
                        # values below 16 in magnitude, one fp32 ulp ~ 1e-6)
PAD_FILL = -1e30


def _ops():
    from emo_disentanger_amd import ops
    return ops


def _tol(dt):           # the per-dtype bound of tests/test_gpu_kernels.py
    return 2e-5 if dt == torch.float32 else 3e-2


def _close(got, ref, dt):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    s = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= _tol(dt) * max(s, 1e-6), 'max err %.3e vs scale %.3e (tol %.1e)' % (err, s, _tol(dt))


def _ld_padded(V):
    """Row stride of the padded layout: 512 (engine.logit_pad's width for V <= 512); a wider vocabulary cannot sit in 512 columns and takes
    logit_pad's rule for it (next multiple of 128)."""
    return 512 if V <= 512 else (V + 127) // 128 * 128


def _case(M, V, ignore, seed=1):
    """fp32 logits (randn x 3), targets with ignored rows, and rows with duplicated maxima / duplicated target values."""
    from emo_disentanger_amd.engine import LOGIT_PAD_FILL
    assert LOGIT_PAD_FILL == PAD_FILL
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(M, V, generator=g) * 3
    tgt = torch.randint(0, V - 1, (M,), generator=g)
    for r in range(0, M, 5):                       # ties
        t = int(tgt[r])
        kind = (r // 5) % 4
        if kind == 0:                              # duplicated maximum, the target is the FIRST of the two -> rank 0
            j = (t + 1 + r) % V
            lo, hi = min(t, j), max(t, j)
            if lo != hi:
                tgt[r] = lo
                logits[r, lo] = logits[r, hi] = float(logits[r].max()) + 1.0
        elif kind == 1:                            # duplicated maximum, the target is the SECOND -> rank 1
            j = (t + 7 + r) % V
            lo, hi = min(t, j), max(t, j)
            if lo != hi:
                tgt[r] = hi
                logits[r, lo] = logits[r, hi] = float(logits[r].max()) + 1.0
        elif kind == 2:                            # the target's value duplicated on both sides of it
            if 0 < t < V - 1:
                logits[r, t - 1] = logits[r, t]
                logits[r, t + 1] = logits[r, t]
                logits[r, 0] = logits[r, t]
        else:                                      # a whole run of equal values around the target
            a, b = max(0, t - 70), min(V, t + 70)
            logits[r, a:b] = logits[r, t]
    if M > 1:
        tgt[1::9] = ignore                         # ignored rows, the last row among them when it falls on the stride
    if M >= 257:
        tgt[-1] = ignore
    return logits, tgt


def _reference(logits, tgt, ignore):
    """float64 on the CPU from the same fp32 values."""
    l = logits.double()
    M, V = l.shape
    logp = torch.log_softmax(l, -1)
    lse = torch.logsumexp(l, -1)
    p = logp.exp()
    entropy = -(p * logp).sum(-1)
    kept = tgt != ignore
    ts = torch.where(kept, tgt, torch.zeros_like(tgt))
    lt = l.gather(1, ts[:, None])
    col = torch.arange(V)[None, :]
    rank = (l > lt).sum(1) + ((l == lt) & (col < ts[:, None])).sum(1)
    rank = torch.where(kept, rank, torch.full_like(rank, -1))
    nll = torch.where(kept, -logp.gather(1, ts[:, None])[:, 0], torch.zeros(M, dtype=torch.float64))
    return nll, lse, rank, entropy


def _device_logits(logits, padded):
    """contiguous [M, V] on the device, or the [:, :V] view of a [M, ld] buffer whose pad columns hold LOGIT_PAD_FILL"""
    M, V = logits.shape
    if not padded:
        return logits.cuda()
    buf = torch.full((M, _ld_padded(V)), PAD_FILL, dtype=torch.float32)
    buf[:, :V] = logits
    return buf.cuda()[:, :V]


@pytest.mark.parametrize('ignore_kind', ['pad', 'torch'])
@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('V', [200, 327, 370, 512, 1000])
@pytest.mark.parametrize('M', [1, 257, 4096])
def test_token_scores_match_float64(M, V, padded, ignore_kind):
    ops = _ops()
    ignore = V - 1 if ignore_kind == 'pad' else -100          # the models' ignore_index (the pad token, a real column) / F.cross_entropy's default
    logits, tgt = _case(M, V, ignore)
    nll_r, lse_r, rank_r, ent_r = _reference(logits, tgt, ignore)
    dl = _device_logits(logits, padded)
    assert dl.stride(0) == (_ld_padded(V) if padded else V)
    out = ops.token_scores(dl, tgt.cuda(), ignore, want=('lse', 'rank', 'entropy'))
    torch.cuda.synchronize()
    nll, lse, rank, ent = out['nll'].cpu(), out['lse'].cpu(), out['rank'].cpu(), out['entropy'].cpu()
    assert rank.dtype == torch.int32 and nll.shape == lse.shape == rank.shape == ent.shape == (M,)
    errs = [float((got.double() - ref).abs().max()) for got, ref in ((nll, nll_r), (lse, lse_r), (ent, ent_r))]
    print('M %d V %d padded %d ignore %s: max |err| nll %.3e lse %.3e entropy %.3e' % (M, V, padded, ignore_kind, *errs))
    assert torch.equal(rank.long(), rank_r), 'rank differs on %d rows' % int((rank.long() != rank_r).sum())
    assert errs[0] <= ROW_TOL and errs[1] <= ROW_TOL and errs[2] <= ROW_TOL, errs
    kept = tgt != ignore
    assert bool((nll[~kept] == 0).all()) and bool((rank[~kept] == -1).all())
    # rank 0 <=> the argmax kernel returns the target.  With ignore_index = -100 that is literally every row (an ignored row has rank -1 and a
    # target no argmax can equal); with the pad token as ignore_index an ignored row is defined to be rank -1 whatever its argmax, so the
    # equivalence is asserted on the scored rows and the ignored ones were checked above.
    am = ops.argmax(logits.cuda()).cpu()
    hit = am == tgt
    if ignore_kind == 'torch':
        assert torch.equal(rank == 0, hit)
    else:
        assert torch.equal((rank == 0)[kept], hit[kept])
    # only nll is mandatory: the same launch with fewer outputs returns the same bits
    only = ops.token_scores(dl, tgt.cuda(), ignore, want=())
    assert set(only) == {'nll'} and torch.equal(only['nll'].cpu(), nll)


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('V', [200, 327, 370, 512])
@pytest.mark.parametrize('M', [1, 257, 4096])
def test_token_scores_lse_is_bitwise_the_training_kernels(M, V, padded):
    # same register layout and reduction order as emo_xent_fwd on both of its paths (M >= 1024: register rows, below: the generic kernel)
    ops = _ops()
    logits, tgt = _case(M, V, V - 1, seed=3)
    lse_t, acc = ops.xent_fwd(logits.cuda(), tgt.cuda(), V - 1)
    out = ops.token_scores(_device_logits(logits, padded), tgt.cuda(), V - 1, want=('lse',))
    assert torch.equal(out['lse'], lse_t)
    kept = (tgt != V - 1)
    assert int(acc[1]) == int(kept.sum())
    assert abs(float(out['nll'].double().sum() / kept.sum()) - float(acc[0] / acc[1])) < 1e-5


@pytest.mark.parametrize('V', EDGE_VS)
@pytest.mark.parametrize('M', EDGE_MS)
def test_lse_bits_are_equal_across_entries_at_every_dispatch_edge(M, V):
    """emo_xent_fwd takes the register kernels from M = 1024, emo_token_scores at any M; both take NV = 6 up to V = 384, NV = 8 up to V = 512 and
    the memory kernel above.  So M = 1023 compares the memory kernel of one entry with the register kernel of the other, M = 1025 the odd tail,
    V = 513 the two memory kernels.  Shifted rows and -inf holes included; once on contiguous logits and once on a [M, V + 8] view."""
    ops = _ops()
    l, tgt = _xent_case(M, V, seed=M + V)
    tgt[::7] = -100
    lse_t, _ = ops.xent_fwd(l.cuda(), tgt.cuda(), -100)
    assert bool(torch.isfinite(lse_t).all())
    wide = torch.full((M, V + 8), PAD_FILL, dtype=torch.float32)
    wide[:, :V] = l
    for dl in (l.cuda(), wide.cuda()[:, :V]):
        lse_s = ops.token_scores(dl, tgt.cuda(), -100, want=('lse',))['lse']
        bad = (lse_s.view(torch.int32) != lse_t.view(torch.int32)).nonzero().view(-1)
        assert bad.numel() == 0, 'ld %d: %d rows differ, first %s' % (dl.stride(0), bad.numel(), bad[:8].tolist())


@pytest.mark.parametrize('V', [65, 384, 513])
def test_rank_zero_is_exactly_where_argmax_is_the_target(V):
    """The identity emo_hip.h states under rank[m], on the planted ties of the edges file (two lanes, one lane, first and last column, tie of three,
    all equal, all -inf, -inf but one) at M = 1025: it follows from the two definitions for any input without NaN, so nothing is approximate."""
    ops = _ops()
    M, pad = 1025, 2
    l = _argmax_case(M, V, seed=M * 7 + V)
    am = ops.argmax(l.cuda()).cpu()
    g = torch.Generator().manual_seed(1)
    tgt = torch.where(torch.rand(M, generator=g) < 0.7, am, torch.randint(0, V, (M,), generator=g))
    hit = am == tgt
    assert 0 < int(hit.sum()) < M and bool(hit[4]) == (int(tgt[4]) == 0)          # row 4 is all -inf: argmax 0
    rank = ops.token_scores(l.cuda(), tgt.cuda(), -100, want=('rank',))['rank'].cpu()
    assert torch.equal(rank == 0, hit), 'rows %s' % ((rank == 0) != hit).nonzero().view(-1)[:8].tolist()
    counts = ops.accuracy_counts(l.cuda(), tgt.cuda(), None, None, pad).cpu().tolist()
    assert counts[:2] == [int((tgt != pad).sum()), int((hit & (tgt != pad)).sum())]


@pytest.mark.parametrize('padded', [False, True])
@pytest.mark.parametrize('M,V', [(1, 327), (257, 200), (257, 1000), (4096, 327), (4096, 512), (1027, 700)])
def test_xent_bwd_rows_matches_autograd_and_the_scalar_kernel(M, V, padded):
    ops = _ops()
    ignore = V - 1
    logits, tgt = _case(M, V, ignore, seed=5)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(M, generator=g)
    lg = logits.clone().requires_grad_(True)
    (torch.nn.functional.cross_entropy(lg, tgt, ignore_index=ignore, reduction='none') * w).sum().backward()
    dlog = _device_logits(logits, padded)
    sc = ops.token_scores(dlog, tgt.cuda(), ignore, want=('lse',))
    for dt in DT:
        dl = ops.xent_bwd_rows(dlog, tgt.cuda(), sc['lse'], w.cuda(), ignore, dt)
        assert dl.dtype == dt and dl.shape == (M, (V + 7) // 8 * 8)
        assert dl.shape[1] == V or float(dl[:, V:].abs().max()) == 0.0
        _close(dl[:, :V], lg.grad, dt)
        wide = ops.xent_bwd_rows(dlog, tgt.cuda(), sc['lse'], w.cuda(), ignore, dt, ld_out=_ld_padded(V) + 128)
        assert wide.shape[1] == _ld_padded(V) + 128 and float(wide[:, V:].abs().max()) == 0.0 and torch.equal(wide[:, :V], dl[:, :V])
        # a constant per-row gradient is the scalar upstream gradient of emo_xent_bwd
        c = torch.full((M,), 0.37, device='cuda')
        rows = ops.xent_bwd_rows(dlog, tgt.cuda(), sc['lse'], c, ignore, dt)
        scalar = ops.xent_bwd(logits.cuda(), tgt.cuda(), sc['lse'], c[:1].clone(), ignore, dt)
        assert torch.equal(rows, scalar)


def test_token_scores_refuses_bad_arguments():
    ops = _ops()
    from emo_disentanger_amd._lib import EmoError
    l = torch.zeros(4, 16, device='cuda')
    t = torch.zeros(4, dtype=torch.int64, device='cuda')
    with pytest.raises(ValueError):
        ops.token_scores(l, t, -100, want=('logprob',))
    with pytest.raises(AssertionError):
        ops.token_scores(l, t, -100, V=17)
    with pytest.raises(EmoError):
        ops.token_scores(l.cpu(), t, -100)
