"""GPU: classifier-free valence guidance end to end (generate_lead_sheets(guidance=, uncond=)) on the small Transformer-XL of
tests/test_gpu_stage1_batch.py (and, for step='one_launch', the two-layer d 512 model of tests/test_gpu_stage1_one_launch.py), three primers of
which one is unguided:
  - the guided LeadSheetLoop, stepped eagerly, against a loop WITHOUT guidance over the same 2n - 1 rows whose logits the test overwrites with
    the NumPy float32 combination after every model step (the followers' uniform columns and emotion mode set to their leaders'): next inputs,
    state, ids and the running count identical at every step (the keys are made likely, so the key rule has keys to reject and primers to re-feed);
  - the graph-replayed run and generate_lead_sheets give the eager ids; under both steps no pair parts and the followers are gone;
  - the unguided piece of a guided call has the ids of the call without guidance, as has every piece at scale 0;
  - 'logp_uncond' for the guided pieces alone; best_of = 2 as pairs, by either ranking;
  - the command line: --guidance S [--uncond EVENT] writes lead sheets, and its refusals.
The golden vocabulary has no Emotion_None: the tests rename one tag of it (the models' weights are synthetic, a name means nothing to them)."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SCALES = [1.5, None, 0.7]
STREAMS = [  # primer, representation, key_determine, max_bars, max_events, prompt_bars
    (['Emotion_Q1'], 'functional', 'rule', 3, 40, None),
    (['Emotion_Negative'], 'functional', 'rule', 3, 36, None),
    (['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M'], 'functional', None, 3, 44, 1),
]


def _with_none(e2i, tag):
    """The vocabulary with the tag `tag` renamed to Emotion_None."""
    e2i = {('Emotion_None' if e == tag else e): i for e, i in e2i.items()}
    return e2i, {i: e for e, i in e2i.items()}


def _small():
    from test_gpu_stage1_batch import _fixture
    _, m, e2i, _ = _fixture()                                       # (a model of its own per call)
    with torch.no_grad():                                           # keys likely: the key draw under the rule meets keys, of either mode
        m.dec_out_proj.bias[[i for e, i in e2i.items() if e.startswith('Key_')]] += 6.0
    return (m,) + _with_none(e2i, 'Emotion_Q2')


def _kw(streams=STREAMS, **more):
    cols = list(zip(*streams))
    return dict(dict(representation=list(cols[1]), key_determine=list(cols[2]), max_bars=list(cols[3]), max_events=list(cols[4]), prompt_bars=list(cols[5]),
                     temp=1.2, top_p=0.9, seed=7), **more)


def _combine(logits, ctl):
    """NumPy float32, three separately rounded operations: both rows of a pair get lc + s * (lc - lu)."""
    l = logits.cpu().numpy()
    out = l.copy()
    for r in range(ctl.n):
        if ctl.guided(r):
            lc, lu = l[ctl.guide_cond[r]], l[ctl.guide_uncond[r]]
            d = lc - lu
            m = np.float32(ctl.guide_scale[r]) * d
            out[r] = lc + m
    assert out.dtype == np.float32
    return torch.from_numpy(out).to(logits.device)


def _model_step(loop):
    loop.model.decode_step(loop.tok, loop.mem, logits_out=loop.logits)


def test_the_guided_loop_is_the_plain_loop_on_combined_logits_step_by_step_and_the_graphed_run_agrees(monkeypatch):
    from emo_disentanger_amd import gen_loop as gl, inference as inf, stage1_inference as s1
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    m, e2i, i2e = _small()
    primers = [st[0] for st in STREAMS]
    plan = inf.guidance_plan('t', SCALES, None, e2i, i2e, [[e2i[e] for e in p] for p in primers])
    ctl = gl.draw_controls('t', 3, len(i2e), None, 1.2, 0.9).with_guidance(plan.scales)
    rows = plan.rows(primers, primers)[1]
    none = e2i['Emotion_None']
    assert rows[3:] == [[none], [none] + [e2i[e] for e in primers[2][1:]]] and ctl.followers() == [3, 4]
    kw = _kw([STREAMS[i] for i in (0, 1, 2, 0, 2)])
    with torch.no_grad():
        a = s1.LeadSheetLoop(m, e2i, i2e, rows, guidance=ctl.guide_arg, **kw)
        b = s1.LeadSheetLoop(m, e2i, i2e, rows, **kw)
        # the leaders draw from the table the call without followers builds; the plain loop's followers get their leader's column ...
        assert torch.equal(a.U[:, :3], inf.uniform_table(a.U.shape[0], 3, 7, a.dev)) and not a.U[:, 3:].any()
        b.U.copy_(a.U)
        b.U[:, 3], b.U[:, 4] = a.U[:, 0], a.U[:, 2]
        # ... and their leader's emotion mode, which the guided loop gives them itself (Emotion_None alone has mode 0)
        pa, pb = a.params.cpu().numpy(), b.params.cpu().numpy()
        assert pa[:, s1.P_EMO_MODE].tolist() == [1, 2, 1, 1, 1] and pb[:, s1.P_EMO_MODE].tolist() == [1, 2, 1, 0, 0]
        b.params.copy_(a.params)
        assert a._gargs.guide_cond is not None and b._gargs.guide_cond is None
        steps = rejected = refed = 0
        pos = a.L0
        while int(a.running.item()) > 0 and pos < a.max_len:
            assert torch.equal(a.logits, b.logits), steps                       # the two models are fed the same tokens
            b.logits.copy_(_combine(b.logits, ctl))
            s0 = a.state.cpu().numpy().copy()
            a.grammar()
            b.grammar()
            for k in ('tok', 'state', 'seq', 'running'):
                assert torch.equal(getattr(a, k), getattr(b, k)), (steps, k)
            st = a.state.cpu().numpy()
            drew = st[:, s1.S_DRAWS] > s0[:, s1.S_DRAWS]
            rejected += int((drew & (st[:, s1.S_LEN] == s0[:, s1.S_LEN]))[[0, 3]].all())
            refed += int((drew & (st[:, s1.S_ACCEPTED] == 0) & (st[:, s1.S_FEED] == 1))[[0, 3]].all())
            for c, f in ((0, 3), (2, 4)):                                       # the pair after every launch: the first token apart
                assert np.array_equal(st[c], st[f]), (steps, c)
            _model_step(a)
            _model_step(b)
            pos += 1
            steps += 1
        assert int(a.running.item()) == 0 and steps > 20
        state, seq = a.state.cpu().numpy(), a.seq.cpu().numpy()
        for c, f in ((0, 3), (2, 4)):
            assert np.array_equal(state[c], state[f]) and np.array_equal(seq[c, 1:], seq[f, 1:]) and seq[c, 0] != seq[f, 0] and seq[f, 0] == none
        c = s1.LeadSheetLoop(m, e2i, i2e, rows, guidance=ctl.guide_arg, **kw)
        c.run(use_graph=True)
        assert torch.equal(c.seq, a.seq) and torch.equal(c.state, a.state)
    print('[stage1 guidance] steps %d, launches in which pair 0 rejected a draw %d, of them with a primer re-feed %d' % (steps, rejected, refed))
    got, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, guidance=SCALES, **_kw())
    ids = lambda rs: [r if isinstance(r, list) else type(r) for r in rs]       # noqa: E731
    assert ids(got) == ids(c.results()[:3]) and len(got) == 3
    # the guidance moved a draw; the unguided piece is the one of the call without guidance
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **_kw())
    assert ids(got[1:2]) == ids(plain[1:2]) and (ids(got[:1]) != ids(plain[:1]) or got[2] != plain[2])


def _one_launch_model():
    from test_gpu_stage1_one_launch import _loop_model
    m, e2i, _ = _loop_model()
    return (m,) + _with_none(e2i, 'Emotion_Q3')


STREAMS_1L = [(['Emotion_Q1'], 'functional', None, 3, 40, None), (['Emotion_Q2'], 'functional', 'rule', 4, 36, None),
              (['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_0_1'], 'functional', None, 3, 44, 1)]


@pytest.mark.parametrize('step', ['chain', 'one_launch'])
def test_no_pair_parts_under_either_step_and_the_unguided_pieces_are_those_of_the_plain_call(step, monkeypatch):
    from emo_disentanger_amd import stage1_inference as s1
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    m, e2i, i2e = _one_launch_model()
    primers = [st[0] for st in STREAMS_1L]
    kw = _kw(STREAMS_1L, step=step)
    base, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **kw)
    got, _, sc = s1.generate_lead_sheets(m, e2i, i2e, primers, guidance=[1.5, None, 1.5], return_scores=True, **kw)
    same = lambda x, y: x == y if isinstance(x, list) else type(x) is type(y)       # noqa: E731  (a key error is a result too)
    assert len(got) == 3 and len(sc) == 3 and not any('lock-step' in str(x) for x in got if isinstance(x, Exception))      # no pair parted
    assert isinstance(got[0], list) and isinstance(got[2], list)                   # (no key rule on the guided pieces: nothing to fail on)
    assert same(got[1], base[1]) and (got[0] != base[0] or got[2] != base[2])
    for i, (ids, s) in enumerate(zip(got, sc)):
        if not isinstance(ids, list):
            continue
        assert ids[:len(primers[i])] == [e2i[e] for e in primers[i]] and len(s['logp']) == len(ids)
        assert ('logp_uncond' in s) == (i != 1)
        if i != 1:
            lu, lc = s['logp_uncond'], s['logp']
            assert lu.shape == lc.shape and np.array_equal(np.isnan(lu), np.isnan(lc)) and (~np.isnan(lc)).sum() >= 1
            assert not np.array_equal(lu[~np.isnan(lu)], lc[~np.isnan(lc)]) and (lu[~np.isnan(lu)] <= 0).all()
    # scale 0, for one piece or for all: the ids of the call without guidance
    mixed, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, guidance=[0, 1.5, 0.0], uncond='Emotion_Positive', **kw)
    assert mixed[0] == base[0] and mixed[2] == base[2] and not (isinstance(mixed[1], Exception) and 'lock-step' in str(mixed[1]))
    for off in (None, 0, [None, 0.0, None]):
        assert all(same(x, y) for x, y in zip(s1.generate_lead_sheets(m, e2i, i2e, primers, guidance=off, **kw)[0], base))


def test_best_of_returns_pairs_by_either_ranking(monkeypatch):
    from emo_disentanger_amd import stage1_inference as s1
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    m, e2i, i2e = _small()
    primers = [st[0] for st in STREAMS]
    for by in ('forward', 'draws'):
        out, _, picks, sc = s1.generate_lead_sheets(m, e2i, i2e, primers, guidance=SCALES, best_of=2, best_by=by, return_scores=True, **_kw())
        assert len(out) == 3 and len(picks) == 3 and len(sc) == 3
        for i, p in enumerate(picks):
            assert len(p['candidates']) == 2 and len(p['scores']) == 2
            assert out[i] is p['candidates'][p['chosen']] or out[i] == p['candidates'][p['chosen']]
            for cand, s in zip(p['candidates'], p['scores']):
                assert not (isinstance(cand, Exception) and 'lock-step' in str(cand)), cand
                if isinstance(cand, list):
                    assert ('logp_uncond' in s) == (i != 1) and cand[:len(primers[i])] == [e2i[e] for e in primers[i]]
        assert any(isinstance(c, list) and not np.isnan(x) for p in picks for c, x in zip(p['candidates'], p['nll_mean']))
        assert isinstance(out[2], list) and 'logp_uncond' in sc[2]                  # (piece 2 runs without the key rule)


def test_command_line_writes_guided_lead_sheets(tmp_path, capsys):
    import yaml
    from emo_disentanger_amd import stage1_inference as s1
    from oracle.txl_ref import make_state_dict_txl
    g = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'txl_generate.json')))
    events = ['Emotion_None' if e == 'Emotion_Q2' else e for e in g['events'] if e != 'PAD_None']
    vocab = tmp_path / 'dictionary.pkl'
    pickle.dump(({e: i for i, e in enumerate(events)}, {i: e for i, e in enumerate(events)}), open(vocab, 'wb'))
    V = len(events) + 1
    sd = make_state_dict_txl(V, 2, 4, 64, 128, seed=3, scale=2.0)
    for e in events:                                              # keys and bars likely, so that the key rule passes and bars appear
        if e.startswith('Key_') or e == 'Bar_None':
            sd['dec_out_proj.bias'][events.index(e)] += 6.0
    torch.save(sd, tmp_path / 'params.pt')
    conf = {'device': 'cuda', 'model': {'d_word_embed': 64, 'pre_lnorm': True,
                                        'decoder': {'n_layer': 2, 'n_head': 4, 'd_model': 64, 'd_ff': 128, 'dropout': 0.1, 'mem_len': 0, 'tgt_len': 64}},
            'data': {'vocab_path': str(tmp_path / 'dictionary.pkl')}}
    yaml.safe_dump(conf, open(tmp_path / 'conf.yaml', 'w'))
    base = ['-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '-m', 'lead_sheet', '-i', str(tmp_path / 'params.pt'), '-n', '2', '--streams', '4',
            '--dtype', 'fp32']
    for name, flags in (('none', ['--guidance', '1.5']), ('contrast', ['--guidance', '1.5', '--uncond', 'Emotion_Q1'])):
        out = tmp_path / name
        s1.main(base + ['-o', str(out)] + flags)
        files = sorted(os.listdir(out))
        assert 1 <= len(files) <= 4 and all(f.startswith('samp_0') and f.endswith('_roman.txt') for f in files), capsys.readouterr().out
        for f in files:
            lines = open(out / f).read().splitlines()
            assert lines and lines[0].startswith('Key_') and not any(x.startswith('Emotion_') for x in lines)
    for bad in (['--guidance', '1.5', '--slots', '2'], ['--guidance', '-1'], ['--uncond', 'Emotion_None']):
        with pytest.raises(SystemExit):
            s1.main(base + ['-o', str(tmp_path / 'bad')] + bad)
    with pytest.raises(ValueError, match='not an event'):
        s1.main(base + ['-o', str(tmp_path / 'bad2'), '--guidance', '1.5', '--uncond', 'Emotion_Q9'])
