"""GPU: the soft sampling controls through the device generation loops — generate_accompaniments / generate_lead_sheets (bias=, top_k=,
min_p=) on the small models of the existing generation tests: the device loops against the host grammar paths on the same draws, id for id
(generate_conditional_batch on both backbones, slots=, best_of=2, a stream that crosses the window under window='host' and 'device';
generate_plain_xl_batch under the chain step, the host rule on the loop's own model step under both steps); per-input controls in a batch
against one-row runs, a guided pair, the hand-over's keyword arguments, a Bar_None bias in stage 1 whose recorded log-probabilities are held
to the unbiased rows, and both command lines under --top-k / --min-p."""
import numpy as np
import pytest
import torch

import test_gpu_stage1_batch as s1b
from test_gpu_generation_controls import KW, _alone, _long, drawn, favourites, s2  # noqa: F401  (s2: the module's fixture)

pytestmark = pytest.mark.gpu


def _soft(e2i):
    return dict(bias=[{'Beat_3': 2.5, e2i['Chord_I_M']: -np.inf}, None, {'Note_Degree_1': -4.0}], top_k=[6, None, 3], min_p=[0.05, 0.2, None])


def test_per_input_soft_controls_equal_one_row_runs_and_bite(s2):
    inf, model, e2i, i2e, leads, primers = s2
    soft = _soft(e2i)
    with torch.no_grad():
        big = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, soft=soft, **KW)
        big.run()
        got = big.results(e2i, i2e, KW['max_events'], False, KW['seed'])
        assert sorted(big.control_tables) == ['bias_of', 'min_p_of', 'tok_bias', 'top_k_of'] and big._gargs.n_biases == 2
        assert big.control_tables['bias_of'].tolist() == [0, -1, 1] and big.control_tables['top_k_of'].tolist() == [6, 0, 3]
        for i in range(3):
            one = _alone(inf, model, e2i, i2e, leads[i], primers[i], big.U[:, i],
                         soft=dict(bias=soft['bias'][i], top_k=soft['top_k'][i], min_p=soft['min_p'][i]), **KW)
            assert one == got[i], i
    api, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, return_scores=True, **soft, **KW)
    assert api == got
    base, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **KW)
    assert all(a != b for a, b in zip(api, base))
    assert e2i['Chord_I_M'] not in {t for _, t in drawn(api[0], sc[0])[0]}           # the -inf entry: never drawn
    # top_k = 1 is greedy: whatever the seed, the same piece
    g1, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, top_k=1, **dict(KW, seed=1))
    g2, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, min_p=1.5, **dict(KW, seed=2))
    assert g1 == g2


def test_the_queue_and_best_of_give_every_job_its_soft_controls(s2):
    inf, model, e2i, i2e, leads, primers = s2
    soft = _soft(e2i)
    lock, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **soft, **KW)
    queue, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, slots=2, **soft, **KW)
    assert queue == lock
    _, _, picks, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=2, best_by='draws', return_scores=True, **soft, **KW)
    for p in picks:
        assert len(p['candidates']) == 2 and not any(isinstance(c, Exception) for c in p['candidates'])
    ban = e2i['Chord_I_M']
    assert all(ban not in {t for _, t in drawn(ids, sc)[0]} for ids, sc in zip(picks[0]['candidates'], picks[0]['scores']))
    loop = inf.AccompanimentLoop(model, e2i, i2e, [x for x in leads for _ in range(2)], [x for x in primers for _ in range(2)],
                                 soft={k: [v for v in vals for _ in range(2)] for k, vals in soft.items()}, **KW)
    assert loop.control_tables['bias_of'].tolist() == [0, 0, -1, -1, 1, 1] and loop.control_tables['top_k_of'].tolist() == [6, 6, 0, 0, 3, 3]


def test_a_guided_follower_stays_with_its_leader_under_the_soft_controls(s2):
    inf, model, e2i, i2e, leads, primers = s2
    soft = _soft(e2i)
    ctl = inf.draw_controls('t', 3, model.n_token, event2idx=e2i, **soft).with_guidance([1.5, 0.0, 1.5])
    assert ctl.tables()['bias_of'].tolist() == [0, -1, 1, 0, 1] and ctl.top_k_at(3) == 6 and ctl.top_k_at(4) == 3
    # (the golden vocabulary has no Emotion_None: Emotion_Q4, id 3, stands in as in test_gpu_guidance_generation.py)
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=[1.5, 0.0, 1.5], uncond=3, **soft, **KW)
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, guidance=[1.5, 0.0, 1.5], uncond=3, **KW)
    assert not any(isinstance(r, Exception) for r in got)          # (check_pairs turns a follower that left its leader into an error)
    assert got[0] != plain[0] and got[2] != plain[2]
    unguided, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **soft, **KW)
    assert got[1] == unguided[1]


@pytest.mark.parametrize('window', ['host', 'device'])
def test_the_soft_controls_hold_behind_the_window(s2, monkeypatch, window):
    inf, model, e2i, i2e = s2[:4]
    leads, primers, kw = _long(s2, monkeypatch)
    base, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='device', return_scores=True, **kw)
    past = favourites([base[0][24:]], [{k: v[24:] for k, v in sc[0].items()}], k=1, spare={e2i['Track_LeadSheet'], e2i['EOS_None']})
    assert past                                                    # a token stream 0 draws behind the window
    bias = [{past[0]: -1e4}, None, None]                           # float32 l - 1e4: exp() of it is 0, the token is never drawn again
    given = {t for bar in leads[0] for t in bar} | {e2i['Track_Full'], e2i['Track_LeadSheet']}
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window=window, bias=bias, top_k=[9, None, None], **kw)
    assert not isinstance(got[0], Exception) and len(got[0]) > 24
    assert past[0] not in set(got[0][24:]) - given
    if window == 'device':
        w_ctl = inf.AccompanimentLoop
        loop = w_ctl(model, e2i, i2e, leads, primers, soft=dict(bias=bias, top_k=[9, None, None]), **kw)
        loop.run()
        loop.results(e2i, i2e, kw['max_events'], False, kw['seed'], window='device')
        w = loop.windowed
        j = w.idx.index(0)
        assert w.control_tables['bias_of'].tolist()[j] == 0 and w.control_tables['top_k_of'].tolist()[j] == 9


def test_the_host_finish_is_handed_the_soft_controls(s2, monkeypatch):
    inf, model, e2i, i2e = s2[:4]
    leads, primers, kw = _long(s2, monkeypatch)
    calls, real = [], inf._resume_windowed

    def spy(*a, **k):
        calls.append((list(a[3].generated[:3]), k))
        return real(*a, **k)

    monkeypatch.setattr(inf, '_resume_windowed', spy)
    inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='host', bias=[{'Beat_3': -3.0}, None, None], top_k=[4, None, None],
                                min_p=[None, None, 0.3], **kw)
    by = {tuple(c[0]): c[1] for c in calls}
    k0 = by[tuple(primers[0])]
    assert k0['top_k'] == 4 and k0['min_p'] == 0.0 and k0['bias'][e2i['Beat_3']] == -3.0 and k0['bias'].dtype == np.float32
    for p in primers[1:]:
        if tuple(p) in by:
            assert 'bias' not in by[tuple(p)]


def test_a_bar_bias_shortens_only_its_job():
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    _, m, e2i, i2e = s1b._fixture('fp32')
    primers = [['Emotion_Positive'], ['Emotion_Positive']]
    kw = dict(representation='functional', key_determine=None, max_bars=6, max_events=120, seed=4)
    bar = e2i['Bar_None']
    with torch.no_grad():
        loop = s1.LeadSheetLoop(m, e2i, i2e, primers, scores=True, soft=dict(bias=[None, inf.event_bias(e2i, {'Bar_None': 6.0})]), **kw)
        loop.U[:, 1] = loop.U[:, 0]                                # two otherwise identical jobs: the same uniforms
        loop.run()
    seq, st = loop.seq.cpu().numpy(), loop.state.cpu().numpy()
    rows = [seq[r, :st[r, 1]].tolist() for r in range(2)]

    def per_bar(ids):
        n = ids.count(bar)
        return (len(ids) - n) / max(n, 1)

    assert rows[0] != rows[1] and rows[1].count(bar) >= 2 and per_bar(rows[1]) < per_bar(rows[0])
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **kw)
    api, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, bias=[None, {'Bar_None': 6.0}], **kw)
    assert api[0] == plain[0]                                      # the unbiased job: the run without `bias`


# ------------------------------------------------------------------------------------------------ the device loops against the host grammar paths
class UDraws:
    """Samplers for a host grammar path that make the device's draws: the d-th call of stream i picks at U[d, i] of the device loop's uniform
    table with sampling.pick_at (the float64 restatement of emo_nucleus_pick), with whatever cut the path hands over as keywords."""

    def __init__(self, U, top_p):
        self.U, self.top_p, self.d = U.cpu().numpy(), top_p, [0] * U.shape[1]

    def samplers(self):
        from emo_disentanger_amd import sampling

        def make(i):
            def f(probs, top_k=0, min_p=0.0):
                u = self.U[self.d[i], i]
                self.d[i] += 1
                return sampling.pick_at(probs, self.top_p, u, top_k, min_p)
            return f
        return [make(i) for i in range(len(self.d))]


def _host2(inf, model, e2i, i2e, leads, primers, soft, kw):
    """generate_conditional_batch under `soft` on the uniforms of the device loop of these inputs."""
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)   # (the loop's uniform table, unused otherwise)
    draws = UDraws(loop.U, kw['top_p'])
    out = inf.generate_conditional_batch(model, e2i, i2e, leads, primers, max_events=kw['max_events'], skip_check=kw['skip_check'], temp=kw['temp'],
                                         top_p=kw['top_p'], samplers=draws.samplers(), **soft)
    return out, draws.d


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_accompaniments_equal_the_host_grammar_path_on_the_same_draws(kind):
    import test_gpu_keep_bars_generation as kb
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = kb._vocab()
    model = kb._tiny(kind)
    leads, primers = kb._inputs(g)
    soft = _soft(e2i)
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **soft, **kb.KW)
    want, draws = _host2(inf, model, e2i, i2e, leads, primers, soft, kb.KW)
    assert got == want                                             # id for id, every stream
    assert min(draws) >= 10 and sum(draws) >= 40                   # (each made draws of its own)
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **kb.KW)
    assert all(a != b for a, b in zip(got, plain))                 # ... and the controls moved every piece
    if kind == 'gpt2':                                             # (rows of a GPT-2 batch do not touch each other: a job's ids do not depend on its slot)
        queued, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, slots=2, **soft, **kb.KW)
        assert queued == want
        rep = lambda v: [x for x in v for _ in range(2)]           # noqa: E731
        _, _, picks, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=2, best_by='draws', return_scores=True, **soft, **kb.KW)
        want2, _ = _host2(inf, model, e2i, i2e, rep(leads), rep(primers), {k: rep(v) for k, v in soft.items()}, kb.KW)
        assert [c for p in picks for c in p['candidates']] == want2


def test_lead_sheets_equal_the_host_grammar_path_on_the_same_draws():
    from emo_disentanger_amd import stage1_inference as s1
    _, m, e2i, i2e = s1b._fixture('fp32')
    primers = [['Emotion_Q1'], ['Emotion_Positive'], ['Emotion_Q2'], ['Emotion_Negative']]
    # (temp / top_p are the key draw's own 1.1 / 0.97: a sampler of the host path is not told which of the two draws it makes)
    kw = dict(representation='functional', key_determine=None, max_bars=5, max_events=80, temp=s1.KEY_TEMP, top_p=s1.KEY_TOP_P)
    soft = dict(bias=[{'Bar_None': 3.0}, None, {'Bar_None': 1.0, e2i['Beat_0']: -np.inf}, None], top_k=[7, 4, None, None], min_p=[None, 0.1, 0.02, None])

    def host(primers, soft, seed):
        loop = s1.LeadSheetLoop(m, e2i, i2e, primers, seed=seed, **kw)
        draws = UDraws(loop.U, kw['top_p'])
        res, _ = s1.generate_plain_xl_batch(m, e2i, i2e, primers, samplers=draws.samplers(), **soft, **kw)
        return [r if isinstance(r, list) else None for r in res], draws.d

    got, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, seed=6, **soft, **kw)
    want, draws = host(primers, soft, 6)
    assert [r if isinstance(r, list) else None for r in got] == want and sum(isinstance(r, list) for r in got) >= 3
    assert min(draws) >= 3 and sum(draws) >= 30                    # (a Bar bias makes a short piece: few draws, each of its own)
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, seed=6, **kw)
    assert got[3] == plain[3] and got[:3] != plain[:3]             # the stream without a control: the run without any
    rep = lambda v: [x for x in v for _ in range(2)]               # noqa: E731
    _, _, picks, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, seed=6, best_of=2, best_by='draws', return_scores=True, **soft, **kw)
    want2, _ = host(rep(primers), {k: rep(v) for k, v in soft.items()}, 6)
    assert [c if isinstance(c, list) else None for p in picks for c in p['candidates']] == want2
    # the queue: every job under its own controls (a job's arithmetic is not lock-step's: held by what the controls forbid and force)
    queued, _, sc = s1.generate_lead_sheets(m, e2i, i2e, primers, seed=6, slots=2, return_scores=True, **soft, **kw)
    ids, s = queued[2], sc[2]
    assert isinstance(ids, list) and e2i['Beat_0'] not in [t for t, r in zip(ids, s['rank']) if r >= 0]
    g1, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, seed=1, slots=2, top_k=1, **kw)
    g2, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, seed=2, slots=2, min_p=[1.5, 2.0, 1.5, 9.0], **kw)
    assert g1 == g2                                                # greedy either way, whatever the uniforms


def test_the_biased_jobs_logp_cells_are_the_models_on_the_unbiased_rows():
    # The loop is stepped by hand (as tests/test_gpu_generation_scores.py steps it): the logits row of every draw is copied in front of the
    # grammar launch, and the cell of each accepted draw of the BIASED job is held to float64 log-softmax of that unbiased row within the
    # bound of the draw scores on a given row (row_tol of tests/test_gpu_draw_scores.py).
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    from test_gpu_draw_scores import row_tol
    from test_gpu_generation_scores import log_softmax64
    _, m, e2i, i2e = s1b._fixture('fp32')
    primers = [['Emotion_Positive'], ['Emotion_Positive']]
    kw = dict(representation='functional', key_determine=None, max_bars=24, max_events=120, seed=4)      # (under the bias a bar is a token or two)
    bar = e2i['Bar_None']
    loop = s1.LeadSheetLoop(m, e2i, i2e, primers, scores=True, soft=dict(bias=[None, inf.event_bias(e2i, {'Bar_None': 6.0})]), **kw)
    hits = bars = 0
    with torch.no_grad():
        while loop._live() > 0 and loop.pos < loop.max_len:
            before, rows = loop.state.cpu().numpy().copy(), loop.logits.clone()
            loop.grammar()
            after, seq = loop.state.cpu().numpy(), loop.seq.cpu().numpy()
            if after[1, s1.S_ACCEPTED] > before[1, s1.S_ACCEPTED]:
                c = int(before[1, s1.S_LEN])
                tok = int(seq[1, c])
                lsm, l64 = log_softmax64(rows[1])
                got = float(loop.score_tables['tok_logp'][1, c].item())
                assert abs(got - lsm[tok]) <= row_tol(l64), (c, tok, got, lsm[tok])
                assert int(loop.score_tables['tok_rank'][1, c].item()) == int((l64 > l64[tok]).sum() + (l64[:tok] == l64[tok]).sum())
                hits += 1
                bars += int(tok == bar)
            if loop._live() == 0:
                break
            m.decode_step(loop.tok, loop.mem, logits_out=loop.logits)
            loop.pos += 1
    assert hits >= 10 and bars >= 2


# ------------------------------------------------------------------------------------------------ the command lines
def _stage2_cli(tmp_path, name, *flags):
    """The set-up of test_gpu_stage2_batch.py's command-line test in a directory of its own -> {file: lines} of the pieces written."""
    import os
    import pickle
    import yaml
    import test_gpu_stage2_batch as s2b
    from emo_disentanger_amd import inference as inf
    from oracle.weights import make_state_dict
    g, _, _ = s2b._vocab()
    root = tmp_path / name
    root.mkdir()
    events = [e for e in g['events'] if e != 'PAD_None']
    e2i = {e: i for i, e in enumerate(events)}
    pickle.dump((e2i, {i: e for e, i in e2i.items()}), open(root / 'dictionary_functional.pkl', 'wb'))
    V = len(events) + 1
    sd = make_state_dict('gpt2', V, 2, 4, 64, 128, seed=3, scale=2.0)
    sd['dec_out_proj.bias'][e2i['Track_LeadSheet']] += 3.0     # bars end soon
    sd['dec_out_proj.bias'][V - 1] -= 30.0                     # the pad id has no event name
    torch.save(sd, root / 'params.pt')
    conf = {'training': {'gpuid': 0}, 'data_loader': {'vocab_path': str(root / 'dictionary_{}.pkl')},
            'model': {'n_layer': 2, 'n_head': 4, 'd_model': 64, 'd_ff': 128, 'd_embed': 64, 'use_segemb': True, 'feature_map': {'n_dims': 32}}}
    yaml.safe_dump(conf, open(root / 'conf.yaml', 'w'))
    out = root / 'gen'
    out.mkdir()
    (out / 'samp_00_Positive_roman.txt').write_text('\n'.join(['Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M', 'Bar_None', 'Beat_4', 'Chord_V_M']) + '\n')
    inf.main(['-m', 'gpt2', '-c', str(root / 'conf.yaml'), '-r', 'functional', '-i', str(root / 'params.pt'), '-o', str(out),
              '--streams', '3', '--dtype', 'fp32', '--max_bars', '8', '--device'] + list(flags))
    return {f: (out / f).read_text().splitlines() for f in sorted(os.listdir(out)) if f.endswith('_full.txt')}


def test_the_stage2_command_line_runs_under_top_k_and_min_p(tmp_path):
    a = _stage2_cli(tmp_path, 'a', '--top-k', '1', '--seed', '1')
    b = _stage2_cli(tmp_path, 'b', '--min-p', '2.0', '--seed', '2')
    c = _stage2_cli(tmp_path, 'c', '--seed', '2')
    assert sorted(a) == ['samp_00_Q1_full.txt', 'samp_00_Q4_full.txt'] and all(len(v) > 8 for v in a.values())
    assert a == b and a != c                                       # greedy under either flag whatever the seed; without them another piece


def _stage1_cli(tmp_path, name, *flags):
    """The set-up of test_gpu_stage1_batch.py's command-line test in a directory of its own -> {file: lines} of the lead sheets written."""
    import json
    import os
    import pickle
    import yaml
    from emo_disentanger_amd import stage1_inference as s1
    from oracle.txl_ref import make_state_dict_txl
    g = json.load(open(os.path.join(s1b.G, 'txl_generate.json')))
    root = tmp_path / name
    root.mkdir()
    events = [e for e in g['events'] if e != 'PAD_None']
    pickle.dump(({e: i for i, e in enumerate(events)}, {i: e for i, e in enumerate(events)}), open(root / 'dictionary.pkl', 'wb'))
    V = len(events) + 1
    sd = make_state_dict_txl(V, 2, 4, 64, 128, seed=3, scale=2.0)
    for e in events:                                              # keys and bars likely, so that the key rule passes and bars appear
        if e.startswith('Key_') or e == 'Bar_None':
            sd['dec_out_proj.bias'][events.index(e)] += 6.0
    torch.save(sd, root / 'params.pt')
    conf = {'device': 'cuda', 'model': {'d_word_embed': 64, 'pre_lnorm': True,
                                        'decoder': {'n_layer': 2, 'n_head': 4, 'd_model': 64, 'd_ff': 128, 'dropout': 0.1, 'mem_len': 0, 'tgt_len': 64}},
            'data': {'vocab_path': str(root / 'dictionary.pkl')}}
    yaml.safe_dump(conf, open(root / 'conf.yaml', 'w'))
    out = root / 'gen'
    s1.main(['-c', str(root / 'conf.yaml'), '-r', 'functional', '-m', 'lead_sheet', '-i', str(root / 'params.pt'), '-o', str(out),
             '-n', '1', '--streams', '2', '--dtype', 'fp32'] + list(flags))
    return {f: (out / f).read_text().splitlines() for f in sorted(os.listdir(out))}


def test_the_stage1_command_line_runs_under_top_k_and_min_p(tmp_path):
    a = _stage1_cli(tmp_path, 'a', '--top-k', '1', '--seed', '1')
    b = _stage1_cli(tmp_path, 'b', '--min-p', '2.0', '--seed', '2')
    c = _stage1_cli(tmp_path, 'c', '--seed', '2')
    assert a and all(f.endswith('_roman.txt') for f in a) and all(len(v) > 2 for v in a.values())
    assert a == b and a != c                                       # greedy under either flag whatever the seed; without them another piece


# ------------------------------------------------------------------------------------------------ past the window, and the one-launch step
class _PhasedSampler:
    """Stream i's sampler for generate_conditional_batch: in the window the device loop's draws (pick_at on column i of its uniform table);
    behind the hand-over (`behind`, set where _resume_windowed takes the stream) what the device path draws with there: NumPy's generator
    seeded [seed, i] for window='host', column j of the windowed loop's own table for window='device'."""

    def __init__(self, U, i, top_p, rng=None, WU=None, j=None):
        self.U, self.i, self.top_p, self.rng, self.WU, self.j = U, i, top_p, rng, WU, j
        self.behind, self.d, self.d2 = False, 0, 0

    def __call__(self, probs, top_k=0, min_p=0.0):
        from emo_disentanger_amd import sampling
        if not self.behind:
            self.d += 1
            return sampling.pick_at(probs, self.top_p, self.U[self.d - 1, self.i], top_k, min_p)
        self.d2 += 1
        if self.rng is not None:
            return sampling.nucleus(probs, self.top_p, rng=self.rng, top_k=top_k, min_p=min_p)
        return sampling.pick_at(probs, self.top_p, self.WU[self.d2 - 1, self.j], top_k, min_p)


@pytest.mark.parametrize('window', ['host', 'device'])
def test_a_stream_that_crosses_the_window_equals_the_host_path(s2, monkeypatch, window):
    inf, model, e2i, i2e = s2[:4]
    leads, primers, kw = _long(s2, monkeypatch)
    soft = _soft(e2i)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, soft=soft, **kw)
    with torch.no_grad():
        loop.run()
        got = loop.results(e2i, i2e, kw['max_events'], False, kw['seed'], window=window)
    crossed = [i for i, x in enumerate(loop.state[:, inf.ACC_S_STATUS].cpu().tolist()) if x == inf.ACC_WINDOW]
    assert 0 in crossed and not any(isinstance(r, Exception) for r in got)
    U = loop.U.cpu().numpy()
    if window == 'host':
        samplers = [_PhasedSampler(U, i, 0.9, rng=np.random.RandomState([kw['seed'], i])) for i in range(3)]
    else:
        w = loop.windowed
        WU = w.U.cpu().numpy()
        samplers = [_PhasedSampler(U, i, 0.9, WU=WU, j=w.idx.index(i) if i in w.idx else None) for i in range(3)]
    real = inf._resume_windowed

    def spy(*a, **k):
        a[8].behind = True                                         # (the stream's own sampler: its draws behind the hand-over)
        return real(*a, **k)

    monkeypatch.setattr(inf, '_resume_windowed', spy)
    want = inf.generate_conditional_batch(model, e2i, i2e, leads, primers, max_events=kw['max_events'], skip_check=False, samplers=samplers, **soft)
    assert got == want                                             # id for id, in front of the window and behind it
    assert sorted(i for i, s in enumerate(samplers) if s.behind) == crossed and samplers[0].d >= 5 and samplers[0].d2 >= 5


@pytest.mark.parametrize('step', ['chain', 'one_launch'])
def test_lead_sheets_under_both_steps_equal_the_host_rule_on_the_same_draws(step):
    # The construction of tests/test_gpu_stage1_keep_bars_generation.py: the loop's own tables and model step (the one-launch stepper where
    # that is the step), every draw on the host by sampling.biased / temperature / pick_at on the loop's uniform table, the key draw at its own
    # temperature and top_p, the grammar by _LeadSheet.
    import test_gpu_stage1_keep_bars_generation as kb1
    from emo_disentanger_amd import inference as inf, sampling, stage1_inference as s1
    m, e2i, i2e, _ = kb1._world()
    primers = [['Emotion_%s' % e] for e in kb1.EMOS]
    n, ME = len(primers), kb1.MAX_EVENTS
    soft = dict(bias=[{'Bar_None': 2.0}, None, inf.event_bias(e2i, {'Beat_': -1.5, 'Key_': 1.0}), {'Bar_None': -np.inf}, None],
                top_k=[5, None, 3, None, 8], min_p=[None, 0.1, 0.05, None, 0.3])
    kw = dict(max_bars=7, max_events=ME, seed=21, step=step)
    got, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **soft, **kw)
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **kw)
    loop = s1.LeadSheetLoop(m, e2i, i2e, primers, soft=soft, **kw)
    ctl, L0, U = loop.job_controls, loop.L0, loop.U.cpu().numpy()
    sheets = [s1._LeadSheet(e2i, primers[i], None, 7, ME, None) for i in range(n)]
    pending = [list(s.tokens[L0:]) for s in sheets]
    tok, draws, live, keys = [s.tokens[L0 - 1] for s in sheets], [0] * n, [True] * n, 0
    logits, pos = loop.logits.clone(), L0
    with torch.no_grad():
        while any(live):
            lg = logits.float().cpu().numpy()
            for i, s in enumerate(sheets):
                if not live[i]:
                    continue
                if pending[i]:
                    tok[i] = pending[i].pop(0)
                    continue
                key = len(s.tokens) == 1
                keys += int(key)
                probs = s1.temperature(sampling.biased(lg[i], ctl.bias_at(i)), s1.KEY_TEMP if key else 1.2)
                word = sampling.pick_at(probs, s1.KEY_TOP_P if key else 0.9, U[draws[i], i], ctl.top_k_at(i), ctl.min_p_at(i))
                draws[i] += 1
                took = s.offer(word, i2e[word])
                if s.stuck or not s.open():
                    live[i] = False
                    continue
                feed = s.tokens if s.accepted == 0 else s.tokens[-1 - (s.chained if took else 0):]
                tok[i], pending[i] = feed[0], list(feed[1:])
            if not any(live):
                break
            assert pos < loop.max_len
            t = torch.tensor(tok, dtype=torch.long, device='cuda')
            logits = (loop.stepper.step(t) if step == 'one_launch' else m.decode_step(t, loop.mem)).clone()
            pos += 1
    want = [None if s.stuck else s.tokens[:-1] for s in sheets]
    assert [r if isinstance(r, list) else None for r in got] == want and sum(r is not None for r in want) >= 4
    assert keys >= n and min(draws) >= 5                           # the key draw of every stream was one of them
    assert sum(a != b for a, b in zip(got, plain)) >= 3            # ... and the controls moved the pieces
