"""GPU: generate_accompaniments(keep=...) end to end, both backbones at the tiny size of tests/test_gpu_stage2_batch.py (fp32), lead sheets of
five bars: an all-kept piece comes back as it is without a step; kept bars {1, 3} stand verbatim in place and the ids are those of the host
grammar (_Stream with keep) driven by the same device draws - compared the way tests/test_gpu_stage2_batch.py compares the device loop to the
host loop: every id of every stream, exactly (share compared: 100 %; these fp32 models leave no bf16 ties to set aside); slots, best_of,
guidance, the refused windows and the --variation-of / --reroll command line."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
KW = dict(max_events=400, skip_check=False, temp=1.2, top_p=0.97, seed=5)


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
        sd['dec_out_proj.bias'][g['events'].index('Track_LeadSheet')] += 3.4 if kind == 'gpt2' else 0.4     # (tests/test_gpu_guidance_generation.py: bars end soon)
        # (no grammar rule keeps a random model from drawing Track_Full inside a bar; such a piece does not parse into bars, a trained model's does)
        sd['dec_out_proj.bias'][g['events'].index('Track_Full')] -= 30.0
        mod.load_state_dict(sd)
        _MODELS[kind] = mod.cuda().eval()
    return _MODELS[kind]


def _inputs(g, n=3):
    lead = [list(b) for b in g['lead']]
    leads = [lead + lead[:2], lead[::-1] + lead[:2], lead[1:] + lead, lead[:2] + lead[::-1]]
    primers = [list(g['primer']), [1, 5, 6], [2, 4, 6], [3, 5, 6]]
    return leads[:n], primers[:n]


def _keep_1_3(inf, e2i, pieces):
    """Bars 1 and 3 of every piece kept (a piece that ended before them: two stand-in bars), the others drawn again."""
    a, b = e2i['Note_Octave_4'], e2i['Chord_I_M']
    keep = []
    for ids in pieces:
        acc = inf.bars_of(ids, e2i)[2]
        keep.append([None, acc[1] if len(acc) > 1 else [a, b], None, acc[3] if len(acc) > 3 else [b], None])
    return keep


def _kept_in_place(inf, e2i, ids, lead, keep):
    primer, bars, acc = inf.bars_of(ids, e2i)
    assert bars == lead[:len(bars)]
    for j, bar in enumerate(keep):
        if bar is not None and j < len(acc) - 1:                 # (the last bar a piece reached may have been cut by max_events)
            assert acc[j] == bar, j
    return len(acc)


def _host_grammar_loop(inf, model, e2i, i2e, leads, primers, keep, U, max_events, skip_check, temp, top_p):
    """_host_grammar_loop of tests/test_gpu_stage2_batch.py with keep: the same engine, ops.sample_nucleus on each stream's own column of U at
    its own draw counter, _Stream (with its kept bars) on the host."""
    from emo_disentanger_amd import ops
    n, W = len(leads), inf.max_dec_inp_len
    dev = U.device
    st = [inf._Stream(e2i, leads[i], primers[i], None, keep[i], max_events) for i in range(n)]
    status = [inf.ACC_DONE if s.done else inf.ACC_RUNNING for s in st]
    draws, fed = [0] * n, 0
    pad = e2i['PAD_None']
    with torch.no_grad():
        eng = inf.make_engine(model, n, redraw=False) if model.kind == 'performer' else inf.GPT2DecodeEngine(model, n, max_len=W)
        L0 = min(len(s.generated) for s in st)
        logits = eng.prefill(torch.tensor([s.generated[:L0] for s in st], device=dev), torch.tensor([s.seg[:L0] for s in st], device=dev))
        for s in st:
            s.consumed = L0
        while True:
            want = [i for i in range(n) if status[i] == inf.ACC_RUNNING and len(st[i].generated) < W and st[i].consumed == len(st[i].generated)]
            assert all(len(s.generated) < W for s in st)
            while want:
                ctr = torch.tensor([min(d, U.shape[0] - 1) for d in draws], device=dev)
                u = U.gather(0, ctr.view(1, n)).view(n).contiguous()
                words = ops.sample_nucleus(logits.contiguous(), temp, top_p, u).cpu().tolist()
                again = []
                for i in want:
                    draws[i] += 1
                    ok = st[i].offer(words[i], e2i, i2e, skip_check, max_events)
                    if st[i].stuck:
                        status[i] = inf.ACC_STUCK
                    elif ok:
                        status[i] = inf.ACC_DONE if st[i].done else status[i]
                    else:
                        again.append(i)
                want = again
            if all(x != inf.ACC_RUNNING for x in status):
                break
            tok, seg = [pad] * n, [1] * n
            for i, s in enumerate(st):
                if status[i] == inf.ACC_RUNNING:
                    tok[i], seg[i] = s.generated[s.consumed], s.seg[s.consumed]
                    s.consumed += 1
            fed += 1
            logits = eng.step(torch.tensor(tok, device=dev), torch.tensor(seg, device=dev)).clone()
    return st, status, draws, fed


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_a_piece_with_all_its_bars_kept_comes_back_as_it_is_without_a_draw(kind):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    model = _tiny(kind)
    leads, primers = _inputs(g)
    pieces, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **KW)
    assert all(isinstance(p, list) for p in pieces)
    parts = [inf.bars_of(p, e2i) for p in pieces]
    assert [p[0] for p in parts] == primers and all(p[1] == ld[:len(p[1])] for p, ld in zip(parts, leads))
    back_leads, keep = [p[1] for p in parts], [p[2] for p in parts]
    got, _, sc = inf.generate_accompaniments(model, e2i, i2e, back_leads, primers, keep=keep, return_scores=True, **KW)
    assert got == pieces
    assert all(np.isnan(s['logp']).all() and (s['rank'] == -1).all() for s in sc)           # nothing was drawn: no score cell
    loop = inf.AccompanimentLoop(model, e2i, i2e, back_leads, primers, keep=keep, **KW)
    assert int(loop.running.item()) == 0 and (loop.state[:, inf.ACC_S_STATUS] == inf.ACC_DONE).all()       # DONE at load
    loop.run()
    state = loop.state.cpu().numpy()
    assert loop.accepted_tokens() == 0 and (state[:, inf.ACC_S_DRAWS] == 0).all()
    assert loop.steps() == int((state[:, inf.ACC_S_CONSUMED] - loop.L0).sum()) == 0         # the step count is the tokens fed: none
    assert loop.results(e2i, i2e, KW['max_events'], False, KW['seed']) == pieces
    # one stream all kept beside two that draw: its row is untouched by the run, the others' steps are the tokens they were fed
    mixed = [keep[0], None, [None, keep[2][1]] if len(keep[2]) > 1 else None]
    loop = inf.AccompanimentLoop(model, e2i, i2e, [back_leads[0], leads[1], leads[2]], primers, keep=mixed, **KW)
    loop.run()
    state = loop.state.cpu().numpy()
    assert state[0, inf.ACC_S_STATUS] == inf.ACC_DONE and state[0, inf.ACC_S_DRAWS] == 0 and state[0, inf.ACC_S_CONSUMED] == loop.L0
    assert loop.results(e2i, i2e, KW['max_events'], False, KW['seed'])[0] == pieces[0]
    assert loop.steps() >= int((state[1:, inf.ACC_S_CONSUMED] - loop.L0).max()) > 0


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_kept_bars_1_and_3_stand_in_place_and_the_ids_are_the_host_grammars_on_the_same_draws(kind):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    model = _tiny(kind)
    leads, primers = _inputs(g)
    pieces, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **KW)
    keep = _keep_1_3(inf, e2i, pieces)
    kw = dict(KW, seed=17)                                               # other draws than the ones that made the pieces
    got, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, keep=keep, return_scores=True, **kw)
    eager, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, keep=keep, use_graph=False, **kw)
    assert eager == got
    reached = [_kept_in_place(inf, e2i, ids, lead, k) for ids, lead, k in zip(got, leads, keep)]
    assert max(reached) >= 4                                             # a kept bar 3 was written by the launch
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, keep=keep, **kw)           # (the loop's uniform table, unused otherwise)
    st, status, draws, fed = _host_grammar_loop(inf, model, e2i, i2e, leads, primers, keep, loop.U, kw['max_events'], False, kw['temp'], kw['top_p'])
    want = [s.generated[:-1] if x == inf.ACC_DONE else s.generated for s, x in zip(st, status)]
    assert got == want                                                   # every id of every stream: share compared 100 %
    loop.run(use_graph=False)
    state = loop.state.cpu().numpy()
    # (the device's last step still runs the model behind the launch that finished the last stream; the host loop stops in front of it)
    assert state[:, inf.ACC_S_DRAWS].tolist() == draws and loop.steps() in (fed, fed + 1)
    # the score cells: one per accepted draw the result keeps, none on a kept token
    for i, (ids, s) in enumerate(zip(got, sc)):
        cells = ~np.isnan(s['logp'])
        # (a DONE stream's result drops its last token, and with it that token's cell where it was drawn)
        assert state[i, inf.ACC_S_ACCEPTED] - int(cells.sum()) in ((0, 1) if status[i] == inf.ACC_DONE else (0,)), i
        primer, bars, acc = inf.bars_of(ids, e2i)
        at = len(primer)
        for j, bar in enumerate(acc):
            at += 1 + len(bars[j]) + 1
            if keep[i][j] is not None and acc[j] == keep[i][j]:
                assert not cells[at:at + len(bar)].any(), (i, j)
            at += len(bar)
    # the host batch loop takes keep the same way (its draws are NumPy's: the kept bars stand, the rest differs)
    host = inf.generate_conditional_batch(model, e2i, i2e, leads, primers, keep=keep, max_events=kw['max_events'], temp=kw['temp'], top_p=kw['top_p'],
                                          seeds=[1, 2, 3])
    for ids, lead, k in zip(host, leads, keep):
        _kept_in_place(inf, e2i, ids, lead, k)


def test_slots_best_of_guidance_and_the_refused_windows():
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    model = _tiny('gpt2')
    leads, primers = _inputs(g, 4)
    pieces, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **KW)
    keep = _keep_1_3(inf, e2i, pieces)
    kw = dict(KW, seed=23)
    lock, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, keep=keep, **kw)
    queued, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, keep=keep, slots=2, **kw)
    assert queued == lock
    # best_of: both candidates of every input hold its kept bars; the ranking is over the re-rolled bars alone
    got, _, picks, sc = inf.generate_accompaniments(model, e2i, i2e, leads[:2], primers[:2], keep=keep[:2], best_of=2, best_by='draws',
                                                    return_scores=True, **kw)
    for i, p in enumerate(picks):
        assert len(p['candidates']) == 2 and got[i] == p['candidates'][p['chosen']]
        for ids in p['candidates']:
            assert isinstance(ids, list)
            _kept_in_place(inf, e2i, ids, leads[i], keep[i])
        assert p['candidates'][0] != p['candidates'][1]
    # guidance: the follower keeps its leader's bars, the pair stays in lock-step (check_pairs leaves no error)
    guided, _ = inf.generate_accompaniments(model, e2i, i2e, leads[:3], primers[:3], keep=keep[:3], guidance=1.5, uncond=3, **kw)
    assert len(guided) == 3
    for ids, lead, k in zip(guided, leads, keep):
        assert isinstance(ids, list), ids
        _kept_in_place(inf, e2i, ids, lead, k)
    for window in ('device', 'rebase'):
        with pytest.raises(ValueError, match='keep is not available with window'):
            inf.generate_accompaniments(model, e2i, i2e, leads, primers, keep=keep, window=window, **kw)


def test_command_line_variation_of_rerolls_the_chosen_bars(tmp_path):
    import yaml
    from emo_disentanger_amd import inference as inf
    from oracle.weights import make_state_dict
    g, _, _ = _vocab()
    events = [e for e in g['events'] if e != 'PAD_None']
    e2i = {e: i for i, e in enumerate(events)}
    pickle.dump((e2i, {i: e for e, i in e2i.items()}), open(tmp_path / 'dictionary_functional.pkl', 'wb'))
    V = len(events) + 1
    sd = make_state_dict('gpt2', V, 2, 4, 64, 128, seed=3, scale=2.0)
    sd['dec_out_proj.bias'][e2i['Track_LeadSheet']] += 3.0     # bars end soon
    sd['dec_out_proj.bias'][V - 1] -= 30.0                     # the pad id has no event name
    sd['dec_out_proj.bias'][e2i['Track_Full']] -= 30.0         # (a random model would draw it inside a bar: such a piece does not parse into bars)
    torch.save(sd, tmp_path / 'params.pt')
    conf = {'training': {'gpuid': 0}, 'data_loader': {'vocab_path': str(tmp_path / 'dictionary_{}.pkl')},
            'model': {'n_layer': 2, 'n_head': 4, 'd_model': 64, 'd_ff': 128, 'd_embed': 64, 'use_segemb': True, 'feature_map': {'n_dims': 32}}}
    yaml.safe_dump(conf, open(tmp_path / 'conf.yaml', 'w'))
    out = tmp_path / 'gen'
    out.mkdir()
    sheet = ['Key_a', 'Bar_None', 'Beat_0', 'Chord_V_M', 'Bar_None', 'Beat_0', 'Chord_I_M', 'Bar_None', 'Beat_8', 'Bar_None', 'Beat_4', 'Chord_V_M']
    (out / 'samp_01_Q2_roman.txt').write_text('\n'.join(sheet) + '\n')
    base = ['-m', 'gpt2', '-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '-i', str(tmp_path / 'params.pt'), '-o', str(out),
            '--streams', '3', '--dtype', 'fp32', '--max_bars', '8', '--device']
    inf.main(base)
    src = out / 'samp_01_Q2_full.txt'
    first = src.read_text().splitlines()
    p0, bars0, acc0 = inf.bars_of([e2i[x] for x in first[1:]], e2i)
    assert len(bars0) >= 3
    inf.main(base + ['--variation-of', str(src), '--reroll', '1:2', '--seed', '7'])
    new = (out / 'samp_01_Q2_full_reroll.txt').read_text().splitlines()
    assert new[0] == first[0] == 'Key_a'
    p1, bars1, acc1 = inf.bars_of([e2i[x] for x in new[1:]], e2i)
    assert (p1, bars1) == (p0, bars0) and len(acc1) == len(acc0) and all(acc1[j] == acc0[j] for j in range(len(acc0)) if j != 1)
    assert src.read_text().splitlines() == first                          # the piece itself is not written over
    for bad in (['--variation-of', str(src)], ['--reroll', '0:1'], ['--variation-of', str(src), '--reroll', '0:1', '--window', 'rebase']):
        with pytest.raises(SystemExit):
            inf.parse_args(base + bad)
    with pytest.raises(ValueError, match='--reroll'):
        inf.main(base + ['--variation-of', str(src), '--reroll', '2:9'])
