"""GPU: generate_lead_sheets(keep=...) end to end on the small Transformer-XL of tests/test_gpu_stage1_one_launch.py.  Five pieces are generated
whole, split with bars_of, and generated again with some of their bars kept (piece 0: its first, a middle and its last bar kept):
  - the ids equal the host rule (_LeadSheet with keep) on the same device draws (ops.sample_nucleus on the loop's own uniform table, the same
    model step), under step='chain' and step='one_launch', and generate_plain_xl_batch(keep=...) replaying those draws gives them again;
  - every kept bar of the result is the input bar token for token (bars_of of the result returns it), every stream ends DONE;
  - slots=2, best_of=2, return_scores=True (the kept cells keep the sentinels, draw_record counts no kept token) and a guided piece;
  - --variation-of / --reroll through main on a file main wrote."""
import functools
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_EVENTS, SEED = 160, 11
EMOS = ['Positive', 'Negative', 'Q1', 'Q2', 'Q3']


@functools.lru_cache(None)
def _world():
    """-> (model, event2idx, idx2event, the five pieces generated whole: ids)."""
    from test_gpu_stage1_one_launch import _model, _sd, _toy_vocab
    from emo_disentanger_amd import stage1_inference as s1
    e2i, i2e = _toy_vocab()
    sd = _sd(2, seed=5)
    for e, i in e2i.items():                                         # keys and beats likely, bars more so: pieces of several short bars
        if e.startswith('Key_') or e.startswith('Beat_'):
            sd['dec_out_proj.bias'][i] += 3.0
        if e == 'Bar_None':
            sd['dec_out_proj.bias'][i] += 6.0
    m = _model(2, 8, 'bf16', sd, max_gen_len=512)
    whole, _ = s1.generate_lead_sheets(m, e2i, i2e, [['Emotion_%s' % e] for e in EMOS], max_bars=7, max_events=MAX_EVENTS, seed=SEED)
    assert all(isinstance(r, list) for r in whole), whole
    return m, e2i, i2e, whole


def _inputs():
    """-> (primers: each piece's head as event names, keep per piece, max_bars per piece, the input bars).  Piece 0 keeps its first, a middle
    and its last bar; piece 1 a chain of two; piece 2 everything but bar 1; piece 3 nothing (keep None); piece 4 its last bar alone."""
    from emo_disentanger_amd import stage1_inference as s1
    m, e2i, i2e, whole = _world()
    primers, keep, max_bars, bars_in = [], [], [], []
    for p, ids in enumerate(whole):
        head, bars, _ = s1.bars_of(ids, e2i)
        assert len(bars) >= 4 and head, (p, len(bars))
        n = len(bars)
        kept = {0: {0, n // 2, n - 1}, 1: {1, 2}, 2: set(range(n)) - {1}, 3: set(), 4: {n - 1}}[p]
        primers.append([i2e[t] for t in head])
        keep.append(None if not kept else [bars[j] if j in kept else None for j in range(n)])
        max_bars.append(n + 1)
        bars_in.append(bars)
    return primers, keep, max_bars, bars_in


def _host_rule_on_device_draws(step, seed):
    """The device loop's own tables and model step, every draw by ops.sample_nucleus, the grammar and the kept bars by _LeadSheet on the host
    -> (ids per stream, the words each stream drew, all streams DONE)."""
    from emo_disentanger_amd import ops, stage1_inference as s1
    m, e2i, i2e, _ = _world()
    primers, keep, max_bars, _ = _inputs()
    loop = s1.LeadSheetLoop(m, e2i, i2e, primers, max_bars=max_bars, max_events=MAX_EVENTS, seed=seed, step=step, keep=keep)
    n, L0 = loop.n, loop.L0
    sheets = [s1._LeadSheet(e2i, primers[i], None, max_bars[i], MAX_EVENTS, keep[i]) for i in range(n)]
    pending = [list(s.tokens[L0:]) for s in sheets]
    tok, draws, live, words = [s.tokens[L0 - 1] for s in sheets], [0] * n, [True] * n, [[] for _ in range(n)]
    logits, pos = loop.logits.clone(), L0
    while any(live):
        u = loop.U.gather(0, torch.tensor(draws, device='cuda').view(1, n)).view(n).contiguous()
        w_main = ops.sample_nucleus(logits, 1.2, 0.9, u).cpu().tolist()
        w_key = ops.sample_nucleus(logits, s1.KEY_TEMP, s1.KEY_TOP_P, u).cpu().tolist()
        for i, s in enumerate(sheets):
            if not live[i]:
                continue
            if pending[i]:
                tok[i] = pending[i].pop(0)
                continue
            word = (w_key if len(s.tokens) == 1 else w_main)[i]
            draws[i] += 1
            words[i].append(word)
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
    return [s.tokens[:-1] for s in sheets], words, all(not s.stuck for s in sheets)


def _check_kept(results, keep, bars_in):
    from emo_disentanger_amd import stage1_inference as s1
    _, e2i, _, _ = _world()
    for p, ids in enumerate(results):
        assert isinstance(ids, list), (p, ids)                         # every stream DONE: none is left out of a comparison
        _, bars, _ = s1.bars_of(ids, e2i)
        for j, bar in enumerate(keep[p] or ()):
            if bar is not None:
                assert bars[j] == bar == bars_in[p][j], (p, j)
        assert len(bars) == len(bars_in[p]) or len(ids) >= MAX_EVENTS, p


@pytest.mark.parametrize('step', ['chain', 'one_launch'])
def test_the_device_loop_equals_the_host_rule_on_the_same_draws(step):
    from emo_disentanger_amd import stage1_inference as s1
    m, e2i, i2e, whole = _world()
    primers, keep, max_bars, bars_in = _inputs()
    kw = dict(max_bars=max_bars, max_events=MAX_EVENTS, seed=SEED + 1, step=step, keep=keep)
    got, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, use_graph=True, **kw)
    eager, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, use_graph=False, **kw)
    ref, words, ok = _host_rule_on_device_draws(step, SEED + 1)
    assert ok and got == ref and eager == got
    _check_kept(got, keep, bars_in)
    assert got[0] != whole[0] and sum(b is None for b in keep[0]) >= 1       # the re-rolled bars were drawn again
    # generate_plain_xl_batch(keep=...), the reference of the rule, replaying the same draws
    its = [iter(w) for w in words]
    host, _ = s1.generate_plain_xl_batch(m, e2i, i2e, primers, max_bars=max_bars, max_events=MAX_EVENTS, keep=keep,
                                         samplers=[(lambda probs, it=it: next(it)) for it in its])
    assert host == got and all(next(it, None) is None for it in its)


def test_slots_best_of_scores_and_a_guided_piece_keep_the_bars():
    from emo_disentanger_amd import scoring, stage1_inference as s1
    m, e2i, i2e, _ = _world()
    primers, keep, max_bars, bars_in = _inputs()
    kw = dict(max_bars=max_bars, max_events=MAX_EVENTS, seed=SEED + 2, keep=keep)
    q, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, slots=2, **kw)
    _check_kept(q, keep, bars_in)
    best, _, picks, sc = s1.generate_lead_sheets(m, e2i, i2e, primers, best_of=2, best_by='draws', return_scores=True, **kw)
    _check_kept(best, keep, bars_in)
    for p, pick in enumerate(picks):
        _check_kept(pick['candidates'], [keep[p]] * 2, [bars_in[p]] * 2)          # every candidate keeps the same bars
    bar = e2i['Bar_None']
    for p, (ids, s) in enumerate(zip(best, sc)):
        drawn = scoring.drawn_mask(s['logp'], s['rank'])
        given = len(primers[p]) + sum(len(b) + 1 for b in keep[p] or () if b is not None)
        if keep[p] and keep[p][-1] is not None:
            given -= 1                                                           # (the Bar that closes a kept last bar is the one the result drops)
        assert int(drawn.sum()) == len(ids) - given == scoring.draw_record(ids, s['logp'], s['rank'], s['entropy'])['n_scored'], p
        head, bars, _ = s1.bars_of(ids, e2i)
        at = len(head)                                                           # (the model may draw in front of its first Bar)
        for j, content in enumerate(bars):                                       # a kept bar's cells, and the Bar that closes it, hold the sentinels
            if j < len(keep[p] or ()) and keep[p][j] is not None:
                span = slice(at + 1, min(at + 1 + len(content) + 1, len(ids)))
                assert not drawn[span].any() and ids[at] == bar, (p, j)
            at += 1 + len(content)
    g, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, guidance=[1.5, None, 0.75, None, None], uncond='Emotion_Q4', **kw)   # (the toy vocabulary has no Emotion_None)
    _check_kept(g, keep, bars_in)
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **kw)
    assert g[1] == plain[1] and g[3] == plain[3] and g[4] == plain[4]            # the unguided pieces of a guided call are those of the plain one


def test_one_stream_keeps_its_primer(tmp_path):
    # one stream, no kept bars: the loop's next-input buffer is a copy of the row's last primer column, never the column itself (with one
    # row the column is contiguous as it stands), so the launch's tok_out does not write into the stream's row
    from emo_disentanger_amd import stage1_inference as s1
    m, e2i, i2e, _ = _world()
    primer = ['Emotion_Q1', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_0_1']
    for step in s1.STEPS:
        loop = s1.LeadSheetLoop(m, e2i, i2e, [primer], max_bars=3, max_events=40, prompt_bars=1, seed=3, step=step)
        assert loop.tok.data_ptr() != loop.seq[:, loop.L0 - 1].data_ptr()
        loop.run(use_graph=False)
        (ids,) = loop.results()
        assert isinstance(ids, list) and len(ids) > len(primer) and ids[:len(primer)] == [e2i[e] for e in primer], (step, ids)


def test_variation_of_through_main_on_a_file_main_wrote(tmp_path):
    import yaml
    from emo_disentanger_amd import stage1_inference as s1
    from oracle.txl_ref import make_state_dict_txl
    from test_gpu_stage1_one_launch import _toy_vocab
    e2i, i2e = _toy_vocab()
    events = [i2e[i] for i in range(len(i2e)) if i2e[i] != 'PAD_None']
    pickle.dump(({e: i for i, e in enumerate(events)}, {i: e for i, e in enumerate(events)}), open(tmp_path / 'dictionary.pkl', 'wb'))
    sd = make_state_dict_txl(len(events) + 1, 2, 4, 64, 128, seed=3, scale=2.0)
    # the remi representation draws no key; Bar by far the likeliest event: the pieces end on max_bars (127 short bars inside 512 events) and
    # the first draw behind a primer is a Bar, so that a re-rolled piece has the head and the bar count of its original
    sd['dec_out_proj.bias'][events.index('Bar_None')] += 8.0
    torch.save(sd, tmp_path / 'params.pt')
    conf = {'device': 'cuda', 'model': {'d_word_embed': 64, 'pre_lnorm': True,
                                        'decoder': {'n_layer': 2, 'n_head': 4, 'd_model': 64, 'd_ff': 128, 'dropout': 0.1, 'mem_len': 0, 'tgt_len': 64}},
            'data': {'vocab_path': str(tmp_path / 'dictionary.pkl')}}
    yaml.safe_dump(conf, open(tmp_path / 'conf.yaml', 'w'))
    out = tmp_path / 'gen'
    base = ['-c', str(tmp_path / 'conf.yaml'), '-m', 'lead_sheet', '-i', str(tmp_path / 'params.pt'), '-o', str(out), '--dtype', 'fp32']
    s1.main(base + ['-r', 'remi', '-n', '1', '--streams', '2'])
    written = sorted(os.listdir(out))
    assert written == ['samp_00_Negative.txt', 'samp_00_Positive.txt']
    src = out / written[0]
    vocab, _, _ = s1.read_vocab(str(tmp_path / 'dictionary.pkl'))
    emotion, head, bars = s1.read_variation(str(src), vocab, ('Positive', 'Negative'))
    redo = [j for j in range(1, len(bars)) if bars[j]][:1] or [1]                # a bar that holds something, if the piece has one
    assert emotion == 'Negative' and len(bars) == 127 and sum(len(b) for b in bars) >= 1
    args = base + ['-r', 'remi', '--variation-of', str(src), '--reroll', '%d:%d,100:103' % (redo[0], redo[0] + 1), '--seed', '5']
    s1.main(args)
    new = out / 'samp_00_Negative_reroll.txt'
    assert os.path.exists(new)
    _, head2, bars2 = s1.read_variation(str(new), vocab, ('Positive', 'Negative'))
    again = set(redo) | {100, 101, 102}
    assert head2 == head and len(bars2) == len(bars)                             # the head token for token, the piece closed where the original did
    assert [b for j, b in enumerate(bars2) if j not in again] == [b for j, b in enumerate(bars) if j not in again]
    stamp = os.path.getmtime(new)
    s1.main(args)                                                               # an output that exists is skipped, as the pieces of a plain run are
    assert os.path.getmtime(new) == stamp
    with pytest.raises(SystemExit):
        s1.main(base + ['-r', 'remi', '--variation-of', str(src), '--reroll', '0:%d' % (len(bars) + 1)])
    with pytest.raises(SystemExit, match='no Key in front of the first Bar'):   # a functional lead sheet opens with its key
        s1.main(base + ['-r', 'functional', '--variation-of', str(src), '--reroll', '1:2'])
