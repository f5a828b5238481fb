"""GPU, model level: compute_loss(reduction='none' | 'sum') on the three models, score_tokens against the oracle forward, the reference's own
per-token losses for GPT-2 (tests/golden/score_gpt2_tiny.npz, tools/make_golden_scores.py), and best-of-N on the device generation loop."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
MAN = json.load(open(os.path.join(G, 'manifest.json')))
TXL = json.load(open(os.path.join(G, 'txl_manifest.json')))
GPT2_CASE = 'gpt2_L2_d64_H4_T128_V327'
PERF_CASE = dict(V=327, L=1, H=2, d=128, dff=256, nf=128, B=2, T=130, seed=5, scale=2.0)       # tests/test_gpu_model.py PERF_CASES[2]
TXL_CASE = sorted(TXL)[0]


def _gpt2(c, dtype):
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from oracle.weights import make_state_dict
    sd = make_state_dict('gpt2', c['V'], c['L'], c['H'], c['d'], c['dff'], n_segment_types=2, seed=c['seed'], scale=c['scale'])
    m = MusicGPT2(c['V'], c['L'], c['H'], c['d'], c['dff'], c['d'], dropout=0.0, use_segment_emb=True, n_segment_types=2, compute_dtype=dtype)
    m.load_state_dict(sd)
    return m.cuda(), sd


def _performer(c, dtype):
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    from oracle.weights import make_state_dict
    sd = make_state_dict('performer', c['V'], c['L'], c['H'], c['d'], c['dff'], favor_feature_dims=c['nf'], seed=c['seed'], scale=c['scale'])
    m = MusicPerformer(c['V'], c['L'], c['H'], c['d'], c['dff'], c['d'], dropout=0.0, favor_feature_dims=c['nf'], use_segment_emb=True,
                       n_segment_types=2, compute_dtype=dtype, redraw='fixed')
    m.load_state_dict(sd)
    return m.cuda(), sd


def _stage2(kind, dtype):
    """(model, state dict, config, batch) of the tiny configurations tests/test_gpu_model.py uses"""
    from oracle.weights import synthetic_batch
    if kind == 'gpt2':
        c = MAN[GPT2_CASE]
        m, sd = _gpt2(c, dtype)
        z = np.load(os.path.join(G, GPT2_CASE + '.npz'))
        b = {'dec_input': torch.from_numpy(z['x']), 'track_mask': torch.from_numpy(z['seg']), 'dec_target': torch.from_numpy(z['tgt'])}
    else:
        c = PERF_CASE
        m, sd = _performer(c, dtype)
        b = synthetic_batch(c['V'], c['B'], c['T'], seed=77, realistic_targets=True)
        b['dec_target'][:, -3:] = 5
    return m, sd, c, b


def _row_tol(logits):
    """1e-5 per row where the logits are below 16 in magnitude (one fp32 ulp ~ 1e-6, tests/test_gpu_token_scores.py); the ulp, and with it the
    bound, grows in proportion above that."""
    return 1e-5 * max(1.0, float(logits.abs().max()) / 16.0)


def _check_reductions(compute_loss, logits, tgt, pad, key):
    """values and input gradients of 'none' / 'sum' against F.cross_entropy on a CPU copy of the same logits; 'mean' untouched"""
    from emo_disentanger_amd import engine, ops
    V = logits.shape[-1]
    lc = logits.detach().cpu().reshape(-1, V).clone().requires_grad_(True)
    tc = tgt.cpu().reshape(-1)
    ref_none = F.cross_entropy(lc, tc, ignore_index=pad, reduction='none')
    w = torch.randn(ref_none.shape, generator=torch.Generator().manual_seed(3))
    (ref_none * w).sum().backward()
    g_none = lc.grad.clone()
    lc.grad = None
    F.cross_entropy(lc, tc, ignore_index=pad, reduction='sum').backward()
    g_sum = lc.grad.clone()
    tol = _row_tol(lc)

    ld = logits.detach().clone().requires_grad_(True)
    out = compute_loss(ld, tgt, reduction='none')
    none = out[key]
    assert out['total_loss'] is none and none.shape == (tc.numel(),) and none.dtype == torch.float32 and none.requires_grad
    err = float((none.detach().cpu().double() - ref_none.detach().double()).abs().max())
    print('none: max |err| %.3e (tol %.1e)' % (err, tol))
    assert err <= tol
    assert bool((none.detach().cpu()[tc == pad] == 0).all())
    (none * w.cuda()).sum().backward()
    gerr = float((ld.grad.cpu().reshape(-1, V) - g_none).abs().max())
    assert gerr <= 2e-5 * float(g_none.abs().max()), gerr            # the fp32 bound of the xent_bwd kernel test

    ld2 = logits.detach().clone().requires_grad_(True)
    s = compute_loss(ld2, tgt, reduction='sum')[key]
    assert s.dim() == 0 and s.requires_grad
    assert float(s) == float(none.detach().sum())                      # 'sum' == 'none'.sum()
    assert abs(float(s) - float(ref_none.detach().double().sum())) <= tol * int((tc != pad).sum())
    s.backward()
    assert float((ld2.grad.cpu().reshape(-1, V) - g_sum).abs().max()) <= 2e-5 * float(g_sum.abs().max())

    mean = compute_loss(logits.detach(), tgt)[key]
    kept = (tgt.reshape(-1) != pad)
    assert abs(float(none.detach()[kept].mean()) - float(mean)) <= 1e-5 * max(1.0, abs(float(mean)))      # a few hundred fp32 terms summed in two orders
    # 'mean' is still XentFn on the forward kernel: that path and no other runs (its two sums are float atomics over the blocks, whose
    # arrival order is free, so two launches on the same input may differ in the last bits: the value is held to 4 fp32 ulp, the route exactly)
    calls = []
    real_fwd, real_rows = ops.xent_fwd, ops.token_scores
    ops.xent_fwd = lambda *a, **k: (calls.append('xent_fwd'), real_fwd(*a, **k))[1]
    ops.token_scores = lambda *a, **k: (calls.append('token_scores'), real_rows(*a, **k))[1]
    try:
        again = compute_loss(logits.detach(), tgt, reduction='mean')[key]
        assert calls == ['xent_fwd']
        compute_loss(logits.detach(), tgt, reduction='none')
        assert calls == ['xent_fwd', 'token_scores']
    finally:
        ops.xent_fwd, ops.token_scores = real_fwd, real_rows
    l2 = logits.detach().reshape(-1, V).contiguous()
    direct = engine.XentFn.apply(l2, tgt.reshape(-1).long(), pad)
    ulp4 = 4 * 1.2e-7 * abs(float(mean))
    assert abs(float(mean) - float(direct)) <= ulp4 and abs(float(mean) - float(again)) <= ulp4
    with pytest.raises(ValueError):
        compute_loss(logits.detach(), tgt, reduction='batchmean')


@pytest.mark.parametrize('kind,dtype', [('gpt2', 'fp32'), ('performer', 'fp32'), ('gpt2', 'bf16'), ('performer', 'bf16')])
def test_stage2_compute_loss_reductions(kind, dtype):
    m, sd, c, b = _stage2(kind, dtype)
    m.train()
    x, seg, tgt = b['dec_input'].cuda(), b['track_mask'].cuda(), b['dec_target'].cuda()
    logits = m(x, seg_inp=seg)
    _check_reductions(m.compute_loss, logits, tgt, c['V'] - 1, 'recons_loss')
    # through the model: the per-row gradient reaches every parameter, and 'sum' is 'mean' times the number of kept targets
    n_kept = int((tgt != c['V'] - 1).sum())
    m.compute_loss(m(x, seg_inp=seg), tgt, reduction='sum')['total_loss'].backward()
    g_sum = {k: p.grad.clone() for k, p in m.named_parameters()}
    m2 = _stage2(kind, dtype)[0].train()                             # (a fresh copy of the same weights: no gradient state shared)
    m2.compute_loss(m2(x, seg_inp=seg), tgt)['total_loss'].backward()
    rel = 2e-3 if dtype == 'fp32' else 6e-2                           # the gradient bounds of tests/test_gpu_model.py
    gmax = max(float(p.grad.abs().max()) for p in m2.parameters()) * n_kept
    for k, p in m2.named_parameters():
        assert torch.isfinite(g_sum[k]).all()
        assert float((g_sum[k] - p.grad * n_kept).abs().max()) <= rel * gmax, k


def test_padded_projection_feeds_the_row_kernels_in_place(monkeypatch):
    # EMO_LOGIT_PAD=1: the bf16 projection writes 512 columns; 'none' reads that buffer and returns its gradient in the same layout
    monkeypatch.setenv('EMO_LOGIT_PAD', '1')
    from emo_disentanger_amd import engine
    m, sd, c, b = _stage2('gpt2', 'bf16')
    m.train()
    x, seg, tgt = b['dec_input'].cuda(), b['track_mask'].cuda(), b['dec_target'].cuda()
    logits = m(x, seg_inp=seg)
    assert engine.padded_logits(logits) is not None and engine.padded_logits(logits).shape[1] == 512
    none = m.compute_loss(logits, tgt, reduction='none')['recons_loss']
    ref = F.cross_entropy(logits.detach().cpu().reshape(-1, c['V']), tgt.cpu().reshape(-1), ignore_index=c['V'] - 1, reduction='none')
    assert float((none.detach().cpu() - ref).abs().max()) <= _row_tol(logits.detach())
    none.sum().backward()
    monkeypatch.setenv('EMO_LOGIT_PAD', '0')
    m2, _, _, _ = _stage2('gpt2', 'bf16')
    m2.train()
    m2.compute_loss(m2(x, seg_inp=seg), tgt, reduction='sum')['recons_loss'].backward()
    gmax = max(float(p.grad.abs().max()) for p in m2.parameters())
    for (k, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        assert float((p.grad - q.grad).abs().max()) <= 2e-2 * gmax, k          # test_padded_output_projection_equals_the_unpadded_one's 2e-2, relative to the largest gradient


def test_stage1_compute_loss_reductions():
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    from oracle.txl_ref import make_state_dict_txl
    c = TXL[TXL_CASE]
    g = np.load(os.path.join(G, TXL_CASE + '.npz'))
    sd = make_state_dict_txl(c['V'], c['L'], c['H'], c['d'], c['dff'], seed=c['seed'], scale=c['scale'])
    m = PlainTransformer(c['d'], c['V'], c['L'], c['H'], c['d'], c['dff'], 0, c['T'], dec_dropout=0.0, pre_lnorm=True, compute_dtype='fp32')
    m.load_state_dict(sd)
    m = m.cuda().train()
    x, tgt = torch.from_numpy(g['x']).cuda(), torch.from_numpy(g['tgt']).cuda()
    logits, _ = m(x, tuple())
    _check_reductions(m.compute_loss, logits, tgt, m.pad_index, 'ce_loss')
    m.compute_loss(m(x, tuple())[0], tgt, reduction='sum')['total_loss'].backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m.parameters())


@pytest.mark.parametrize('kind', ['gpt2', 'performer'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_score_tokens_matches_the_oracle(kind, dtype):
    from emo_disentanger_amd import ops, scoring
    from oracle import model_ref
    m, sd, c, b = _stage2(kind, dtype)
    m.train()                                                        # score_tokens switches to eval and back
    x, seg, tgt = b['dec_input'].cuda(), b['track_mask'].cuda(), b['dec_target'].cuda()
    sc = scoring.score_tokens(m, x, tgt, seg_inp=seg)
    assert m.training
    pad = c['V'] - 1
    with torch.no_grad():
        rl = model_ref.forward(kind, sd, b['dec_input'], b['track_mask'], c['L'], c['H'], c['d'], form='quadratic').double()
    logp = torch.log_softmax(rl, -1)
    mask = b['dec_target'] != pad
    ref_lp = torch.where(mask, logp.gather(-1, torch.where(mask, b['dec_target'], torch.zeros_like(b['dec_target']))[..., None])[..., 0],
                         torch.zeros((), dtype=torch.float64))
    ref_ent = -(logp.exp() * logp).sum(-1)
    assert sc.logprob.shape == sc.rank.shape == sc.entropy.shape == tgt.shape and torch.equal(sc.mask.cpu(), mask)
    lp, ent = sc.logprob.cpu().double(), sc.entropy.cpu().double()
    e_lp, e_ent = float((lp - ref_lp).abs().max()), float((ent - ref_ent).abs().max())
    print('%s %s: max |err| logprob %.3e entropy %.3e' % (kind, dtype, e_lp, e_ent))
    if dtype == 'fp32':
        tol = 2e-4 if kind == 'gpt2' else 3e-4                       # the fp32 logit bounds (rtol = atol) of tests/test_gpu_model.py for these configurations
        np.testing.assert_allclose(lp.numpy(), ref_lp.numpy(), rtol=tol, atol=tol)
        np.testing.assert_allclose(ent.numpy(), ref_ent.numpy(), rtol=tol, atol=tol)
    else:
        assert e_lp <= 3e-2 and e_ent <= 3e-2                         # its bf16 bound (the loss bound, here per token)
    assert bool((sc.logprob[~sc.mask] == 0).all()) and bool((sc.rank[~sc.mask] == -1).all())
    # rank is self-consistent with the model's own logits: 0 exactly where the argmax kernel returns the target
    m.eval()
    with torch.no_grad():
        own = m(x, seg_inp=seg).reshape(-1, c['V']).contiguous()
    hit = (ops.argmax(own) == tgt.reshape(-1)).view_as(tgt)
    assert torch.equal((sc.rank == 0)[sc.mask], hit[sc.mask])
    only = scoring.score_tokens(m, x, tgt, seg_inp=seg, want=('logprob',))
    assert only.rank is None and only.entropy is None and torch.equal(only.logprob, sc.logprob)


def test_score_pieces_records_on_the_device():
    from emo_disentanger_amd import scoring
    m, sd, c, b = _stage2('gpt2', 'fp32')
    pad = c['V'] - 1
    res = scoring.score_pieces(m.eval(), [b, b], pad)
    sc = scoring.score_tokens(m, b['dec_input'].cuda(), b['dec_target'].cuda(), seg_inp=b['track_mask'].cuda())
    B = b['dec_input'].shape[0]
    assert len(res['pieces']) == 2 * B and res['corpus']['n_pieces'] == 2 * B
    for i, r in enumerate(res['pieces'][:B]):
        mk = sc.mask[i]
        assert r['n_scored'] == int(mk.sum()) and abs(r['nll_sum'] + float(sc.logprob[i][mk].double().sum())) < 1e-6
        assert abs(r['top1'] - float((sc.rank[i][mk] == 0).double().mean())) < 1e-12
        assert abs(r['top5'] - float((sc.rank[i][mk] < 5).double().mean())) < 1e-12
        assert abs(r['entropy_mean'] - float(sc.entropy[i][mk].double().mean())) < 1e-9
        assert res['pieces'][B + i]['nll_sum'] == r['nll_sum']
    assert abs(res['corpus']['nll_mean'] + float(sc.logprob[sc.mask].double().mean())) < 1e-9


def test_gpt2_per_token_loss_matches_the_reference_fixture():
    z = np.load(os.path.join(G, 'score_gpt2_tiny.npz'))
    c = {k: (float(v) if k == 'scale' else int(v)) for k, v in zip(z['cfg_keys'].tolist(), z['cfg_vals'].tolist())}
    m, _ = _gpt2(c, 'fp32')
    m.eval()
    x, seg, tgt = [torch.from_numpy(z[k]).cuda() for k in ('x', 'seg', 'tgt')]
    with torch.no_grad():
        logits = m(x, seg_inp=seg)
        none = m.compute_loss(logits, tgt, reduction='none')['recons_loss']
        total = m.compute_loss(logits, tgt, reduction='sum')['recons_loss']
    assert none.shape == z['nll_none'].shape
    np.testing.assert_allclose(none.cpu().numpy(), z['nll_none'], rtol=2e-4, atol=2e-4)      # the golden-logits tolerance of tests/test_gpu_model.py
    assert abs(float(total) - float(z['nll_sum'])) <= 2e-4 * float(z['nll_sum'])
    assert abs(float(m.compute_loss(logits, tgt)['recons_loss']) - float(z['nll_mean'])) <= 1e-4


# ------------------------------------------------------------------------------------------------ best of N
def _gen_vocab():
    g = json.load(open(os.path.join(G, 'generate.json')))
    e2i = {e: i for i, e in enumerate(g['events'])}
    return g, e2i, {i: e for e, i in e2i.items()}


def _tiny(kind, dtype):
    """the tiny generation models of tests/test_gpu_stage2_batch.py"""
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    from oracle.weights import make_state_dict
    m = json.load(open(os.path.join(G, 'generate.json')))['model']
    if kind == 'gpt2':
        sd = make_state_dict('gpt2', m['V'], m['L'], m['H'], m['d'], m['dff'], seed=m['seed'], scale=m['scale'])
        mod = MusicGPT2(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], dropout=0.1, use_segment_emb=True, n_segment_types=2, compute_dtype=dtype)
    else:
        sd = make_state_dict('performer', m['V'], m['L'], m['H'], m['d'], m['dff'], favor_feature_dims=32, seed=m['seed'], scale=m['scale'])
        mod = MusicPerformer(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], favor_feature_dims=32, use_segment_emb=True, n_segment_types=2,
                             compute_dtype=dtype, redraw='fixed')
    mod.load_state_dict(sd)
    return mod.cuda().eval()


def _nll_mean_independent(model, e2i, ids):
    """float64 log-softmax on the CPU of the model's own logits, over the targets the dataset rule gives"""
    from emo_disentanger_amd import scoring
    inp, tgt, seg = scoring.targets_of(ids, e2i, pad_token=model.n_token - 1)
    with torch.no_grad():
        lg = model(torch.from_numpy(inp)[None].cuda(), seg_inp=torch.from_numpy(seg)[None].cuda())[0].cpu().double()
    logp = torch.log_softmax(lg, -1)
    keep = np.flatnonzero(tgt != model.n_token - 1)
    return float(-logp[keep, tgt[keep]].mean())


@pytest.mark.parametrize('kind,dtype', [('gpt2', 'fp32'), ('performer', 'fp32'), ('gpt2', 'bf16')])
def test_best_of_three_returns_the_most_likely_candidate(kind, dtype):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _gen_vocab()
    model = _tiny(kind, dtype)
    lead = [list(b) for b in g['lead']]
    leads = [lead, lead[::-1], lead[:2], lead + lead]
    primers = [list(g['primer']), [1, 5, 6], list(g['primer']), [3, 5, 6]]
    kw = dict(max_events=150, temp=1.2, top_p=0.97, seed=5)
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **kw)
    one = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=1, **kw)
    assert len(one) == 2 and one[0] == plain                         # best_of = 1: today's path, today's draws
    got, _, picks = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=3, **kw)
    assert len(got) == len(picks) == len(leads)
    for i, p in enumerate(picks):
        assert len(p['candidates']) == len(p['nll_mean']) == 3 and got[i] == p['candidates'][p['chosen']]
        assert all(isinstance(cand, list) and cand[:len(primers[i])] == primers[i] for cand in p['candidates'])
        mine = [_nll_mean_independent(model, e2i, cand) for cand in p['candidates']]
        print('lead sheet %d: device %s recomputed %s chosen %d' % (i, ['%.5f' % v for v in p['nll_mean']], ['%.5f' % v for v in mine], p['chosen']))
        # the batched, padded scoring pass and a single-sequence forward agree to the forward's own rounding
        # (fp32: 1e-4, the loss bound of the parity tests; bf16: 3e-2)
        tol = 1e-4 if dtype == 'fp32' else 3e-2
        assert max(abs(a - b) for a, b in zip(mine, p['nll_mean'])) <= tol
        assert p['chosen'] == int(np.argmin(p['nll_mean']))
        if sorted(mine)[1] - sorted(mine)[0] > 2 * tol:              # the recomputed minimum is decided: it is the returned candidate
            assert p['chosen'] == int(np.argmin(mine))
        assert mine[p['chosen']] <= min(mine) + 2 * tol
    assert len({tuple(c) for p in picks for c in p['candidates']}) > len(leads)      # the candidates of a lead sheet are distinct draws
    with pytest.raises(ValueError):
        inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=0, **kw)
