"""GPU: prefill(tok, seg, lens=...) of both decode engines: rows of different lengths in one padded batch, every row stepping on from its
own position.  The reference is the same engine class fed token by token from an empty state; the tolerance is twice the error e0 that the
parent's own prefill (one common length) shows against that token-by-token feed.  Tiny fp32 models of tests/test_gpu_stage2_window.py."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
LENS, T, STEPS = [5, 17, 40], 40, 3


def _tiny(kind):
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    from oracle.weights import make_state_dict
    m = json.load(open(os.path.join(G, 'generate.json')))['model']
    if kind == 'gpt2':
        sd = make_state_dict('gpt2', m['V'], m['L'], m['H'], m['d'], m['dff'], seed=m['seed'], scale=m['scale'])
        mod = MusicGPT2(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], dropout=0.1, use_segment_emb=True, n_segment_types=2, compute_dtype='fp32')
    else:
        sd = make_state_dict('performer', m['V'], m['L'], m['H'], m['d'], m['dff'], favor_feature_dims=32, seed=m['seed'], scale=m['scale'])
        mod = MusicPerformer(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], favor_feature_dims=32, use_segment_emb=True, n_segment_types=2,
                             compute_dtype='fp32', redraw='fixed')
    mod.load_state_dict(sd)
    return mod.cuda().eval()


def _engine(inf, model, n):
    return inf.PerformerDecodeEngine(model, n, redraw=False) if model.kind == 'performer' else inf.GPT2DecodeEngine(model, n, max_len=64)


_CASE = {}


def _case(kind):
    """Model, tokens / segments [3, T + STEPS], and the token-by-token reference: logits[i] = the logits after feeding columns 0 .. i from
    an empty engine (computed once per backbone, shared by the tests, never changed)."""
    if kind not in _CASE:
        from emo_disentanger_amd import inference as inf
        model = _tiny(kind)
        gen = torch.Generator().manual_seed(3)
        tok = torch.randint(0, model.n_token - 1, (3, T + STEPS), generator=gen).cuda()
        seg = torch.randint(0, 2, (3, T + STEPS), generator=gen).cuda()
        eng = _engine(inf, model, 3)
        if kind == 'performer':
            eng.start_empty()
        eng.pos_dev.zero_()
        eng.dev_pos0, eng.pos_auto = 0, True
        ref = [eng.step(tok[:, i].contiguous(), seg[:, i].contiguous(), dev_pos=True).clone() for i in range(T + STEPS)]
        _CASE[kind] = (model, tok, seg, torch.stack(ref))
    return _CASE[kind]


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_varlen_prefill_and_three_steps_equal_the_token_by_token_feed(kind):
    from emo_disentanger_amd import inference as inf
    model, tok, seg, ref = _case(kind)
    # e0: the parent's prefill at the common length T against the same tokens through step
    base = _engine(inf, model, 3)
    e0 = (base.prefill(tok[:, :T].contiguous(), seg[:, :T].contiguous()) - ref[T - 1]).abs().max().item()
    assert e0 > 0
    lens = torch.tensor(LENS, dtype=torch.int32, device='cuda')
    eng = _engine(inf, model, 3)
    got = [eng.prefill(tok[:, :T].contiguous(), seg[:, :T].contiguous(), lens=lens).clone()]
    assert eng.pos_dev.tolist() == LENS and eng.dev_pos0 == 0 and eng.pos == T
    eng.pos_auto = True
    for j in range(STEPS):
        at = lens.long() + j
        got.append(eng.step(tok.gather(1, at.view(-1, 1)).view(-1), seg.gather(1, at.view(-1, 1)).view(-1), dev_pos=True).clone())
    assert eng.pos_dev.tolist() == [x + STEPS for x in LENS]
    worst = 0.0
    for j, g in enumerate(got):
        for b, L in enumerate(LENS):
            want = ref[L - 1 + j, b]
            worst = max(worst, (g[b] - want).abs().max().item())
            assert int(g[b].argmax()) == int(want.argmax()), (j, b)
    print('varlen prefill %s: worst %.3e, e0 %.3e' % (kind, worst, e0))
    assert worst <= 2 * e0, (worst, e0)


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_lens_none_is_the_path_it_was(kind):
    from emo_disentanger_amd import inference as inf
    model, tok, seg, _ = _case(kind)
    a, b = _engine(inf, model, 3), _engine(inf, model, 3)
    # a has seen the new argument, b never does
    a.prefill(tok[:, :T].contiguous(), seg[:, :T].contiguous(), lens=torch.tensor(LENS, dtype=torch.int32, device='cuda'))
    la = a.prefill(tok[:, :T].contiguous(), seg[:, :T].contiguous(), lens=None)
    lb = b.prefill(tok[:, :T].contiguous(), seg[:, :T].contiguous())
    assert torch.equal(la, lb) and a.pos == b.pos == T and torch.equal(a.pos_dev, b.pos_dev)
    for i in range(STEPS):
        sa = a.step(tok[:, T + i].contiguous(), seg[:, T + i].contiguous())
        sb = b.step(tok[:, T + i].contiguous(), seg[:, T + i].contiguous())
        assert torch.equal(sa, sb), i


def test_lens_of_the_wrong_kind_are_refused():
    from emo_disentanger_amd import _lib, inference as inf
    model, tok, seg, _ = _case('gpt2')
    eng = _engine(inf, model, 3)
    with pytest.raises(_lib.EmoError, match='int32'):
        eng.prefill(tok[:, :T].contiguous(), seg[:, :T].contiguous(), lens=torch.tensor(LENS, device='cuda'))
