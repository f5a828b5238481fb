"""GPU: stage-1 lead-sheet scoring through the model — PlainTransformer.forward_windowed against the one-token steps it restates
(generate() + decode_step) and against the pinned oracle driven token by token with memory (oracle/txl_ref.py), score_lead_sheet_tokens
against a float64 log-softmax of the oracle's logits, and generate_lead_sheets(best_of=N)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
# the tiny model of tests/test_gpu_stage1.py (its first fixture case, tests/golden/txl_manifest.json: txl_L2_d64_H4_T32_V50), constructor
# arguments copied from its _model(); fp32, a memory of 48 positions, 150 tokens
C = dict(V=50, L=2, H=4, d=64, dff=128, T=32, scale=8.0, seed=21)
MEM_LEN, T, B = 48, 150, 2
TOKEN_SEED = 3
LENGTHS, PRIMER_LENS, PAD_AT = [150, 97], [1, 5], (1, 60)           # ragged rows, two primer lengths, one PAD inside row 1
LOGIT_TOL = 2e-4      # x the logits' scale, fp32: tests/test_gpu_generate.py holds the one-token steps to the full forward at this bound
ROW_TOL = 1e-5        # absolute, per scored position: the bound tests/test_gpu_token_scores.py holds emo_token_scores to


def _tokens():
    g = torch.Generator().manual_seed(TOKEN_SEED)
    tok = torch.randint(0, C['V'] - 1, (B, T), generator=g)
    for b, n in enumerate(LENGTHS):
        tok[b, n:] = C['V'] - 1
    tok[PAD_AT] = C['V'] - 1
    return tok


@functools.lru_cache(None)
def _oracle():
    """(state dict, tokens [B, T], logits [T, B, V] of oracle.txl_ref.forward fed one token at a time with a memory of MEM_LEN hidden states).
    Computed once on the CPU and shared by the tests below; none of them changes it."""
    from oracle import txl_ref
    sd = txl_ref.make_state_dict_txl(C['V'], C['L'], C['H'], C['d'], C['dff'], seed=C['seed'], scale=C['scale'])
    tok = _tokens()
    x = tok.t().contiguous()
    rows, mems = [], None
    with torch.no_grad():
        for i in range(T):
            lg, mems = txl_ref.forward(sd, x[i:i + 1], C['L'], C['H'], mems=mems, mem_len=MEM_LEN)
            rows.append(lg[0])
    return sd, tok, torch.stack(rows, 0)


@functools.lru_cache(None)
def _model():
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    sd = _oracle()[0]
    m = PlainTransformer(C['d'], C['V'], C['L'], C['H'], C['d'], C['dff'], MEM_LEN, C['T'], dec_dropout=0.1, pre_lnorm=True, compute_dtype='fp32')
    m.load_state_dict(sd)
    return m.cuda().eval()


@functools.lru_cache(None)
def _windowed():
    m, tok = _model(), _oracle()[1]
    return m.forward_windowed(tok.t().contiguous().cuda()).cpu()          # [T, B, V]


def test_forward_windowed_equals_the_one_token_steps():
    m, (_, tok, _) = _model(), _oracle()
    x = tok.t().contiguous().cuda()
    lg0, mem = m.generate(x[:1], tuple())                                 # (stream 0's logits, memory of both streams)
    steps = [m.decode_step(x[i], mem).clone() for i in range(1, T)]
    steps = torch.stack(steps, 0).cpu()                                   # [T - 1, B, V]
    got = _windowed()
    assert got.shape == (T, B, C['V']) and got.dtype == torch.float32
    scale = float(steps.abs().max())
    e0, e = float((got[0, 0] - lg0.cpu()).abs().max()), float((got[1:] - steps).abs().max())
    print('windowed forward vs one-token steps: first position %.3e, rest %.3e (scale %.3e)' % (e0, e, scale))
    assert e0 <= LOGIT_TOL * scale and e <= LOGIT_TOL * scale
    assert int(got[0, 0].argmax()) == int(lg0.argmax()) and torch.equal(got[1:].argmax(-1), steps.argmax(-1))
    # the band is not the causal forward: past the window the unwindowed logits differ
    m0 = type(m)(C['d'], C['V'], C['L'], C['H'], C['d'], C['dff'], 0, C['T'], dec_dropout=0.1, pre_lnorm=True, compute_dtype='fp32')
    m0.load_state_dict(_oracle()[0])
    with torch.no_grad():
        full = m0.cuda().eval()(x, tuple())[0].cpu()
    assert float((full[:MEM_LEN + 1] - got[:MEM_LEN + 1]).abs().max()) <= LOGIT_TOL * scale
    assert float((full[MEM_LEN + 1:] - got[MEM_LEN + 1:]).abs().max()) > LOGIT_TOL * scale


def test_forward_windowed_equals_the_oracle_token_by_token():
    ref, got = _oracle()[2], _windowed()
    scale = float(ref.abs().max())
    e = float((got - ref).abs().max())
    print('windowed forward vs oracle with memory: %.3e (scale %.3e)' % (e, scale))
    assert e <= LOGIT_TOL * scale
    assert torch.equal(got.argmax(-1), ref.argmax(-1))


def test_forward_windowed_refuses_training_mode_and_an_empty_window():
    m, tok = _model(), _oracle()[1]
    x = tok.t().contiguous().cuda()
    with pytest.raises(ValueError):
        m.forward_windowed(x, window=0)
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m.forward_windowed(x)
    finally:
        m.eval()
    w = m.forward_windowed(x, window=T + 5).cpu()                         # an explicit window wins over dec_mem_len
    assert float((w - _windowed()).abs().max()) > 0


def _float64_reference():
    """log-probability, rank and margin of every next-token target under the oracle's logits, in float64."""
    _, tok, ref = _oracle()
    l = ref.double().permute(1, 0, 2)                                      # [B, T, V]
    logp = torch.log_softmax(l, -1)
    nxt = torch.cat([tok[:, 1:], torch.full((B, 1), C['V'] - 1)], 1)
    own = l.gather(-1, nxt[..., None])
    lp = logp.gather(-1, nxt[..., None])[..., 0]
    rank = (l > own).sum(-1) + ((l == own) & (torch.arange(C['V']) < nxt[..., None])).sum(-1)
    gap = (l - own).abs()
    gap.scatter_(-1, nxt[..., None], float('inf'))
    return nxt, lp, rank, gap.min(-1).values


def _expected_mask(tok):
    mask = torch.zeros(B, T, dtype=torch.bool)
    for b in range(B):
        mask[b, PRIMER_LENS[b] - 1:LENGTHS[b] - 1] = True
    mask[PAD_AT[0], PAD_AT[1] - 1] = False                                 # its target is PAD
    return mask


def test_score_lead_sheet_tokens_against_float64_of_the_oracle():
    from emo_disentanger_amd import scoring
    m, tok = _model(), _oracle()[1]
    sc = scoring.score_lead_sheet_tokens(m, tok.cuda(), LENGTHS, PRIMER_LENS)
    assert not m.training
    nxt, lp, rank, margin = _float64_reference()
    mask = _expected_mask(tok)
    assert torch.equal(sc.mask.cpu(), mask)                               # before the primer, the last token and past it, PAD targets: not scored
    got_lp, got_rank = sc.logprob.cpu().double(), sc.rank.cpu().long()
    assert float(got_lp[~mask].abs().max()) == 0.0 and bool((got_rank[~mask] == -1).all())
    err = float((got_lp - lp)[mask].abs().max())
    safe = mask & (margin > ROW_TOL)
    print('log-probability vs float64 of the oracle logits: %.3e over %d positions; rank compared at %d of them' % (err, int(mask.sum()), int(safe.sum())))
    assert err <= ROW_TOL
    assert int(safe.sum()) >= 0.9 * int(mask.sum())
    assert torch.equal(got_rank[safe], rank[safe])
    # the per-piece records are the sums of these rows
    recs = scoring.score_lead_sheets(m, [tok[b, :LENGTHS[b]].tolist() for b in range(B)], PRIMER_LENS, batch=2)
    for b, r in enumerate(recs):
        assert r['n_tokens'] == LENGTHS[b] and r['n_scored'] == int(mask[b].sum()) and r['primer_outside_window'] is False
        assert abs(r['nll_sum'] + float(lp[b][mask[b]].sum())) <= ROW_TOL * r['n_scored']


# ------------------------------------------------------------------------------------------------ best of N
def _generator_fixture():
    """The traced tiny generator of tests/test_gpu_stage1.py (tests/golden/txl_generate.json: model, vocabulary), constructor arguments copied."""
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    from oracle.txl_ref import make_state_dict_txl
    g = json.load(open(os.path.join(G, 'txl_generate.json')))
    c = g['model']
    e2i = {e: i for i, e in enumerate(g['events'])}
    i2e = {i: e for e, i in e2i.items()}
    sd = make_state_dict_txl(c['V'], c['L'], c['H'], c['d'], c['dff'], seed=c['seed'], scale=c['scale'])
    m = PlainTransformer(c['d'], c['V'], c['L'], c['H'], c['d'], c['dff'], c['T'], c['T'], dec_dropout=0.1, pre_lnorm=True, compute_dtype='fp32')
    m.load_state_dict(sd)
    return m.cuda().eval(), e2i, i2e


def test_best_of_runs_the_candidates_as_streams_and_keeps_the_likeliest():
    from emo_disentanger_amd import scoring, stage1_inference as s1
    m, e2i, i2e = _generator_fixture()
    primers = [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Positive'], ['Emotion_Negative', 'Key_a']]
    N = 3
    kw = dict(max_bars=4, max_events=60, temp=1.2, top_p=0.9, representation='functional', seed=11)
    res, _, picks = s1.generate_lead_sheets(m, e2i, i2e, primers, best_of=N, **kw)
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, [p for p in primers for _ in range(N)], **kw)
    ok = lambda r: isinstance(r, list)
    assert len(res) == len(picks) == len(primers) and sum(ok(r) for r in plain) >= 6
    same = lambda a, b: a == b if ok(a) or ok(b) else type(a) is type(b)
    for i, p in enumerate(picks):
        assert len(p['candidates']) == len(p['nll_mean']) == N
        for c in range(N):                                                 # candidate c of primer i is stream i * N + c of the plain 12-stream call
            assert same(p['candidates'][c], plain[i * N + c]), (i, c)
        # scores recomputed one candidate at a time, outside the batch the pick was made in
        again = [scoring.score_lead_sheets(m, [cand], [len(primers[i])], batch=1)[0]['nll_mean'] if ok(cand) else float('nan')
                 for cand in p['candidates']]
        finite = [x for x in again if x == x]
        if finite:
            assert p['chosen'] == int(np.nanargmin(again)) and ok(p['candidates'][p['chosen']])
            assert same(res[i], p['candidates'][p['chosen']])
        assert [a != a for a in p['nll_mean']] == [b != b for b in again]      # NaN exactly for the failed candidates
    one, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, best_of=1, **kw)
    none, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **kw)
    assert all(same(a, b) for a, b in zip(one, none)) and sum(ok(r) for r in none) >= 2
