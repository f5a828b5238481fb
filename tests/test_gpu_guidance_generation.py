"""GPU: classifier-free emotion guidance end to end (generate_accompaniments(guidance=, uncond=)) on the small models of
tests/test_gpu_stage2_batch.py, three short synthetic lead sheets of which one is unguided:
  - the guided AccompanimentLoop, stepped eagerly, against a loop WITHOUT guidance over the same 2n - 1 rows whose logits the test overwrites with
    the NumPy float32 combination before every grammar launch: ids and state identical at every step;
  - the graph-replayed run gives the eager ids;
  - the results: followers absent, the pair invariant, 'logp_uncond' for the guided pieces alone, best_of = 2 as pairs, guidance off = the call
    without the argument;
  - window='rebase': a pair crosses the (lowered) window together, stays aligned through the phases and passes the pair check; window='host':
    the same piece holds the EmoError that names window='rebase'.
The golden vocabulary has no Emotion_None: the tests hand Emotion_Q4 over as `uncond`."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
UNCOND = 3                            # Emotion_Q4 stands in for the unconditioned token
SCALES = [1.5, None, 0.7]
KW = dict(max_events=60, skip_check=False, temp=1.2, top_p=0.97, seed=5)
W, KEEP = 96, 48


def _vocab():
    g = json.load(open(os.path.join(G, 'generate.json')))
    e2i = {e: i for i, e in enumerate(g['events'])}
    return g, e2i, {i: e for e, i in e2i.items()}


_MODELS = {}


def _tiny(kind):
    if kind not in _MODELS:
        from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
        from emo_disentanger_amd.model.music_performer import MusicPerformer
        from oracle.weights import make_state_dict
        g = json.load(open(os.path.join(G, 'generate.json')))
        m = g['model']
        if kind == 'gpt2':
            sd = make_state_dict('gpt2', m['V'], m['L'], m['H'], m['d'], m['dff'], seed=m['seed'], scale=m['scale'])
            mod = MusicGPT2(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], dropout=0.1, use_segment_emb=True, n_segment_types=2, compute_dtype='fp32')
        else:
            sd = make_state_dict('performer', m['V'], m['L'], m['H'], m['d'], m['dff'], favor_feature_dims=32, seed=m['seed'], scale=m['scale'])
            mod = MusicPerformer(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], favor_feature_dims=32, use_segment_emb=True, n_segment_types=2,
                                 compute_dtype='fp32', redraw='fixed')
        # (tests/test_gpu_stage2_rebase.py: bars of a dozen or two events, far below the lowered window)
        sd['dec_out_proj.bias'][g['events'].index('Track_LeadSheet')] += 3.4 if kind == 'gpt2' else 0.4
        mod.load_state_dict(sd)
        _MODELS[kind] = mod.cuda().eval()
    return _MODELS[kind]


def _inputs(g):
    lead = [list(b) for b in g['lead']]
    return [lead + lead, lead[::-1], lead[:2]], [list(g['primer']), [1, 5, 6], [2, 4, 6]]


def _guided_rows(inf, gl, e2i, i2e, leads, primers, V):
    plan = inf.guidance_plan('t', SCALES, UNCOND, e2i, i2e, primers)
    ctl = gl.draw_controls('t', len(primers), V, None, KW['temp'], KW['top_p']).with_guidance(plan.scales)
    return plan, ctl, plan.rows(leads, primers)


def _combine(logits, ctl):
    """NumPy float32, three rounded operations: both rows of a pair get lc + s * (lc - lu)."""
    l = logits.cpu().numpy()
    out = l.copy()
    for r in range(ctl.n):
        if ctl.guided(r):
            lc, lu = l[ctl.guide_cond[r]], l[ctl.guide_uncond[r]]
            out[r] = lc + np.float32(ctl.guide_scale[r]) * (lc - lu)
    assert out.dtype == np.float32
    return torch.from_numpy(out).to(logits.device)


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_the_guided_loop_is_the_plain_loop_on_combined_logits_step_by_step_and_the_graphed_run_agrees(kind, monkeypatch):
    from emo_disentanger_amd import gen_loop as gl, inference as inf
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    g, e2i, i2e = _vocab()
    model = _tiny(kind)
    leads, primers = _inputs(g)
    plan, ctl, (leads_x, primers_x) = _guided_rows(inf, gl, e2i, i2e, leads, primers, model.n_token)
    assert len(primers_x) == 5 and primers_x[3] == [UNCOND, 4, 6] and primers_x[4] == [UNCOND, 4, 6] and ctl.followers() == [3, 4]
    with torch.no_grad():
        a = inf.AccompanimentLoop(model, e2i, i2e, leads_x, primers_x, guidance=ctl.guide_arg, redraw=False, **KW)
        b = inf.AccompanimentLoop(model, e2i, i2e, leads_x, primers_x, redraw=False, **KW)
        # the leaders draw from the table the call without followers builds; the plain loop's followers get their leader's column
        assert torch.equal(a.U[:, :3], inf.uniform_table(a.U.shape[0], 3, KW['seed'], a.dev)) and not a.U[:, 3:].any()
        b.U.copy_(a.U)
        b.U[:, 3], b.U[:, 4] = a.U[:, 0], a.U[:, 2]
        assert a._gargs.guide_cond is not None and b._gargs.guide_cond is None
        steps = 0
        while int(a.running.item()) > 0 and steps < 400:
            assert torch.equal(a.logits, b.logits), steps                       # the two engines are fed the same tokens
            b.logits.copy_(_combine(b.logits, ctl))
            a.grammar()
            b.grammar()
            for k in ('tok', 'segv', 'state', 'seq', 'segs', 'running'):
                assert torch.equal(getattr(a, k), getattr(b, k)), (steps, k)
            a.eng.step(a.tok, a.segv, dev_pos=True, logits_out=a.logits)
            b.eng.step(b.tok, b.segv, dev_pos=True, logits_out=b.logits)
            steps += 1
        assert int(a.running.item()) == 0 and steps > 20
        state, seq = a.state.cpu().numpy(), a.seq.cpu().numpy()
        for c, f in ((0, 3), (2, 4)):
            assert np.array_equal(state[c], state[f]) and np.array_equal(seq[c, 1:], seq[f, 1:]) and seq[c, 0] != seq[f, 0]
        c = inf.AccompanimentLoop(model, e2i, i2e, leads_x, primers_x, guidance=ctl.guide_arg, redraw=False, **KW)
        c.run(use_graph=True)
        assert torch.equal(c.seq, a.seq) and torch.equal(c.state[:, :6], a.state[:, :6]) and torch.equal(c.state[:, 6:], a.state[:, 6:])
    # the guidance moved a draw
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **KW)
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=SCALES, uncond=UNCOND, **KW)
    assert got == c.results(e2i, i2e, KW['max_events'], False, KW['seed'])[:3]
    assert got[0] != plain[0] or got[2] != plain[2]


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_results_drop_the_followers_and_carry_the_unconditioned_logp(kind, monkeypatch):
    from emo_disentanger_amd import inference as inf
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    g, e2i, i2e = _vocab()
    model = _tiny(kind)
    leads, primers = _inputs(g)
    got, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=SCALES, uncond=UNCOND, return_scores=True, **KW)
    bare, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=SCALES, uncond=UNCOND, **KW)
    assert len(got) == 3 and len(sc) == 3 and all(isinstance(x, list) for x in got) and bare == got      # (a pair that parted would hold an EmoError)
    for i, (ids, s) in enumerate(zip(got, sc)):
        assert ids[:3] == primers[i] and len(s['logp']) == len(ids)
        assert ('logp_uncond' in s) == (i != 1)
        if i != 1:
            lu, lc = s['logp_uncond'], s['logp']
            assert lu.shape == lc.shape and np.array_equal(np.isnan(lu), np.isnan(lc)) and (~np.isnan(lc)).sum() >= 1
            assert not np.array_equal(lu[~np.isnan(lu)], lc[~np.isnan(lc)]) and (lu[~np.isnan(lu)] <= 0).all()
    # best_of = 2: every candidate is a pair; three pieces come back, by either ranking
    for by in ('forward', 'draws'):
        out, _, picks = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=SCALES, uncond=UNCOND, best_of=2, best_by=by, **KW)
        assert len(out) == 3 and len(picks) == 3
        for i, p in enumerate(picks):
            assert len(p['candidates']) == 2 and all(isinstance(x, list) and x[:3] == primers[i] for x in p['candidates'])
            assert out[i] == p['candidates'][p['chosen']] and not any(np.isnan(p['nll_mean']))
    # guidance off: the ids of the call without the argument
    base, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **KW)
    for off in (None, 0, [None, 0.0, None]):
        assert inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=off, **KW)[0] == base


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_a_pair_crosses_the_window_together_under_rebase_and_is_refused_by_the_host_window(kind, monkeypatch):
    from emo_disentanger_amd import _lib, gen_loop as gl, inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', W)
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    model = _tiny(kind)
    lead = [list(b) for b in g['lead']]
    leads, primers = [(lead * 4)[:12], lead[:2]], [list(g['primer']), [1, 5, 6]]
    kw = dict(KW, max_events=330)
    scale = 1.5 if kind == 'performer' else 0.5
    scales = [scale, None]
    plan = inf.guidance_plan('t', scales, UNCOND, e2i, i2e, primers)
    ctl = gl.draw_controls('t', 2, model.n_token, None, kw['temp'], kw['top_p']).with_guidance(plan.scales)
    leads_x, primers_x = plan.rows(leads, primers)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads_x, primers_x, guidance=ctl.guide_arg, redraw=False, scores=True, **kw)
    loop.run()
    status = loop.state[:, inf.ACC_S_STATUS].cpu().tolist()
    assert status[0] == inf.ACC_WINDOW and status[2] == inf.ACC_WINDOW                # the pair reached the window in the same launch
    out = loop.results(e2i, i2e, 330, False, kw['seed'], window='rebase', rebase_keep=KEEP)
    rl = loop.windowed
    assert isinstance(rl, inf.RebaseLoop) and rl.phases >= 1 and rl.idx == [0, 2]
    assert rl.controls.guide_arg == ([0, 0], [1, 1], [scale, scale]) and rl._gargs.guide_cond is not None      # the pair, renumbered, in the phases' block
    assert loop.statuses[0] == loop.statuses[2]
    # the rows of the pair as the last phase left them: word for word alike, the emotion token apart
    home = rl.seq_pp[rl.home[0]].cpu().numpy()
    assert rl.home[0] == rl.home[1] and np.array_equal(rl.state[0].cpu().numpy(), rl.state[1].cpu().numpy())
    assert np.array_equal(home[0, 1:], home[1, 1:]) and home[0, 0] == 0 and home[1, 0] == UNCOND
    assert torch.equal(rl.arch_len[0], rl.arch_len[1]) and torch.equal(rl.arch_tok[0], rl.arch_tok[1]) and int(rl.arch_len[0]) > 0
    folded, sc = inf.check_pairs(out, loop.statuses, loop.scores(out), ctl, plan.emo_pos)
    if isinstance(out[0], list):
        assert isinstance(out[2], list) and len(out[0]) > W
        assert len(out[0]) == len(out[2]) and out[0][1:] == out[2][1:] and out[0][0] == 0 and out[2][0] == UNCOND
        assert folded == out[:2] and 'logp_uncond' in sc[0] and len(sc[0]['logp_uncond']) == len(out[0])
    else:
        # (the small random model may leave a bar open for longer than the lowered window: then both rows end on that error, in the same phase)
        assert kind != 'performer' and 'a bar longer than the window' in str(out[0]) and 'a bar longer than the window' in str(out[2])
        assert folded[0] is out[0] and sc[0] is None
    # the public call: the same piece; with the host window, the refusal
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=scales, uncond=UNCOND, window='rebase', rebase_keep=KEEP, **kw)
    assert got == out[:2]
    host, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=scales, uncond=UNCOND, **kw)
    assert isinstance(host[0], _lib.EmoError) and "window='rebase'" in str(host[0]) and host[1] == got[1]
