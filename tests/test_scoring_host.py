"""Host-side logic of the scoring module (no GPU): targets_of against EventPieceDataset._targets, the record / summary arithmetic, the
command line with a stub scorer, and the best-of-N choice."""
import json
import math
import os
import pickle

import numpy as np
import pytest
import torch


def _vocab():
    names = ['Emotion_Q1', 'Key_C', 'Tempo_110', 'Track_LeadSheet', 'Track_Full', 'Bar_None', 'EOS_None'] + ['Beat_%d' % i for i in range(4)] + \
            ['Note_%d' % i for i in range(6)] + ['Chord_I_M', 'Chord_V_M', 'Duration_1', 'Duration_2']
    e2i = {e: i for i, e in enumerate(names)}
    return e2i, {i: e for e, i in e2i.items()}


def _piece(e2i, n_bars, seed=0, eos=True):
    """(lead_pos, full_pos, ids) in the on-disk layout: header, then per bar a lead-sheet part and a full part; EOS closes the last span."""
    rng = np.random.default_rng(seed)
    ev = ['Emotion_Q1', 'Key_C', 'Tempo_110']
    lead_pos, full_pos = [], []
    for _ in range(n_bars):
        s = len(ev)
        ev += ['Track_LeadSheet', 'Bar_None']
        for _ in range(int(rng.integers(1, 4))):
            ev += ['Beat_%d' % rng.integers(0, 4), 'Chord_I_M', 'Note_%d' % rng.integers(0, 6)]
        lead_pos.append((s, len(ev)))
        s = len(ev)
        ev.append('Track_Full')
        for _ in range(int(rng.integers(2, 6))):
            ev += ['Beat_%d' % rng.integers(0, 4), 'Note_%d' % rng.integers(0, 6), 'Duration_%d' % rng.integers(1, 3)]
        full_pos.append((s, len(ev)))
    if eos:
        ev.append('EOS_None')
        full_pos[-1] = (full_pos[-1][0], len(ev))
    return lead_pos, full_pos, np.array([e2i[e] for e in ev], dtype=int)


def _dataset_targets(e2i, inp, lead_pos, full_pos):
    from emo_disentanger_amd.data import EventPieceDataset
    ds = object.__new__(EventPieceDataset)
    ds.pad_token, ds.eos_token, ds.predict_key = len(e2i), e2i['EOS_None'], False
    return ds._targets(inp, lead_pos, full_pos, 0)


@pytest.mark.parametrize('n_bars,eos', [(1, True), (4, True), (7, True), (5, False)])
def test_targets_of_is_the_dataset_rule(n_bars, eos):
    from emo_disentanger_amd import scoring
    e2i, _ = _vocab()
    lead_pos, full_pos, ids = _piece(e2i, n_bars, seed=n_bars, eos=eos)
    want_t, want_m = _dataset_targets(e2i, ids, lead_pos, full_pos)
    inp, tgt, seg = scoring.targets_of(list(ids), e2i)
    assert inp.dtype == tgt.dtype == seg.dtype == np.int64
    assert np.array_equal(inp, ids) and np.array_equal(tgt, want_t) and np.array_equal(seg, want_m)
    pad = len(e2i)
    assert tgt[-1] == e2i['EOS_None']                              # the last span's last target, with or without an EOS token in the list
    assert (tgt[seg == 0] == pad).all() and (tgt[seg == 1] != pad).all()
    a = full_pos[0][0]
    assert tgt[a] == ids[a + 1] and tgt[a - 1] == pad              # Track_Full predicts the first accompaniment token; the lead sheet predicts nothing


def test_targets_of_cuts_a_long_piece_like_the_dataset():
    from emo_disentanger_amd import scoring
    e2i, _ = _vocab()
    lead_pos, full_pos, ids = _piece(e2i, 9, seed=3)
    want_t, want_m = _dataset_targets(e2i, ids, lead_pos, full_pos)
    W = len(ids) // 2
    inp, tgt, seg = scoring.targets_of(list(ids), e2i, max_len=W)
    assert len(inp) == len(tgt) == len(seg) == W
    assert np.array_equal(inp, ids[:W]) and np.array_equal(tgt, want_t[:W]) and np.array_equal(seg, want_m[:W])
    assert (tgt != len(e2i)).sum() < (want_t != len(e2i)).sum()     # fewer targets scored than the piece has
    # a list without any Track_Full span scores nothing; an explicit pad id is honoured
    inp, tgt, seg = scoring.targets_of([e2i['Emotion_Q1'], e2i['Track_LeadSheet'], e2i['Bar_None']], e2i, pad_token=99)
    assert (tgt == 99).all() and (seg == 0).all()


def test_batches_pad_to_the_longest_of_each_group():
    from emo_disentanger_amd import scoring
    e2i, _ = _vocab()
    lists = [list(_piece(e2i, n, seed=n)[2]) for n in (2, 5, 3)]
    got = list(scoring.batches_of(lists, e2i, max_len=60, batch=2, ids=['a', 'b', 'c']))
    assert [b['piece_id'] for b in got] == [['a', 'b'], ['c']] and [b['length'] for b in got] == [[len(lists[0]), len(lists[1])], [len(lists[2])]]
    pad = len(e2i)
    b0 = got[0]
    T = min(60, max(len(lists[0]), len(lists[1])))
    assert b0['dec_input'].shape == b0['dec_target'].shape == b0['track_mask'].shape == (2, T)
    n0 = len(lists[0])
    assert (b0['dec_input'][0, n0:] == pad).all() and (b0['dec_target'][0, n0:] == pad).all() and (b0['track_mask'][0, n0:] == 0).all()
    assert np.array_equal(b0['dec_target'][0, :n0].numpy(), scoring.targets_of(lists[0], e2i)[1])


def test_records_and_token_weighted_summary():
    from emo_disentanger_amd import scoring
    r1 = scoring.piece_record('a', 50, 10, 20.0, 4, 8, 15.0)
    r2 = scoring.piece_record('b', 90, 30, 30.0, 3, 9, 60.0)
    assert r1 == {'id': 'a', 'n_tokens': 50, 'n_scored': 10, 'nll_sum': 20.0, 'nll_mean': 2.0, 'ppl': math.exp(2.0), 'top1': 0.4, 'top5': 0.8,
                  'entropy_mean': 1.5}
    c = scoring.corpus_summary([r1, r2])
    assert c['n_pieces'] == 2 and c['n_tokens'] == 140 and c['n_scored'] == 40 and 'id' not in c
    assert c['nll_sum'] == 50.0 and c['nll_mean'] == 1.25 and c['ppl'] == math.exp(1.25)
    assert abs(c['top1'] - 7 / 40) < 1e-12 and abs(c['top5'] - 17 / 40) < 1e-12 and abs(c['entropy_mean'] - 75 / 40) < 1e-12
    empty = scoring.piece_record('c', 5, 0, 0.0, 0, 0, 0.0)
    assert empty['n_scored'] == 0 and math.isnan(empty['nll_mean']) and math.isnan(empty['ppl'])
    assert scoring.corpus_summary([r1, empty])['nll_mean'] == 2.0


def _stub_scorer(calls):
    from emo_disentanger_amd import scoring

    def scorer(model, dec_input, dec_target, seg_inp=None, want=scoring.WANT, pad_token=None):
        calls.append((tuple(dec_input.shape), pad_token))
        assert seg_inp is not None and seg_inp.shape == dec_input.shape
        mask = dec_target != pad_token
        lp = torch.where(mask, -0.5 - 0.01 * dec_target.float(), torch.zeros(()))
        rank = torch.where(mask, dec_target % 7, torch.full((), -1, dtype=torch.int64)).int()
        return scoring.TokenScores(lp, rank, torch.full(dec_target.shape, 1.25), mask)
    return scorer


def _workspace(tmp_path, e2i, i2e, max_len=40):
    with open(tmp_path / 'dictionary.pkl', 'wb') as f:
        pickle.dump((e2i, i2e), f)
    conf = {'data_loader': {'vocab_path': str(tmp_path / 'dictionary.pkl'), 'data_path': str(tmp_path), 'train_split': 'x', 'val_split': 'y'},
            'model': {'max_len': max_len}, 'training': {'gpuid': 0}}
    import yaml
    with open(tmp_path / 'conf.yaml', 'w') as f:
        yaml.safe_dump(conf, f)
    files = []
    for k, n_bars in enumerate((2, 6, 3)):
        ids = _piece(e2i, n_bars, seed=10 + k, eos=False)[2]
        p = tmp_path / ('samp_%02d_Q1_full.txt' % k)
        p.write_text('\n'.join(['Key_C'] + [i2e[int(t)] for t in ids]) + '\n')      # the layout inference.main writes: key line first
        files.append((str(p), ids))
    return files


def test_main_writes_scores_json_with_a_stub_scorer(tmp_path):
    from emo_disentanger_amd import scoring
    e2i, i2e = _vocab()
    files = _workspace(tmp_path, e2i, i2e)
    calls, seen = [], {}

    def load_model(args, conf, n_token):
        seen['n_token'], seen['dtype'] = n_token, args.dtype
        return torch.nn.Linear(1, 1)

    out = tmp_path / 'scores.json'
    res = scoring.main(['-m', 'gpt2', '-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '--params', 'ckpt.pt', '--dtype', 'fp32', '--batch', '2',
                        '--files'] + [f for f, _ in files] + ['-o', str(out), '--per-token', str(tmp_path / 'tok')],
                       scorer=_stub_scorer(calls), load_model=load_model)
    pad = len(e2i)
    assert seen == {'n_token': pad + 1, 'dtype': 'fp32'}
    assert len(calls) == 2 and all(p == pad for _, p in calls) and calls[0][0][0] == 2 and calls[1][0][0] == 1
    on_disk = json.loads(out.read_text())
    assert on_disk['pieces'] == res['pieces'] and set(on_disk) == {'pieces', 'corpus', 'model'}
    assert on_disk['model'] == {'type': 'gpt2', 'params': 'ckpt.pt', 'dtype': 'fp32', 'max_len': 40}
    keys = ['id', 'n_tokens', 'n_scored', 'nll_sum', 'nll_mean', 'ppl', 'top1', 'top5', 'entropy_mean']
    for (path, ids), rec in zip(files, on_disk['pieces']):
        assert list(rec) == keys and rec['id'] == os.path.basename(path)[:-4]
        _, tgt, _ = scoring.targets_of(list(ids), e2i, max_len=40)
        kept = tgt[tgt != pad]
        assert rec['n_tokens'] == len(ids) and rec['n_scored'] == len(kept)
        if len(ids) > 40:
            assert rec['n_scored'] < (scoring.targets_of(list(ids), e2i)[1] != pad).sum()
        want = float((0.5 + 0.01 * kept.astype(np.float32)).sum())
        assert abs(rec['nll_sum'] - want) < 1e-4 and abs(rec['nll_mean'] - want / len(kept)) < 1e-5
        assert abs(rec['ppl'] - math.exp(rec['nll_mean'])) < 1e-9
        assert abs(rec['top1'] - (kept % 7 == 0).mean()) < 1e-12 and abs(rec['top5'] - (kept % 7 < 5).mean()) < 1e-12
        assert abs(rec['entropy_mean'] - 1.25) < 1e-12
        stem = os.path.join(str(tmp_path / 'tok'), rec['id'])
        lp, rk = np.load(stem + '.logprob.npy'), np.load(stem + '.rank.npy')
        assert lp.shape == rk.shape == np.load(stem + '.entropy.npy').shape and (rk[:min(len(ids), 40)][tgt == pad] == -1).all()
    assert max(len(ids) for _, ids in files) > 40                   # one piece of the three is cut to max_len
    c = on_disk['corpus']
    assert c['n_pieces'] == 3 and c['n_scored'] == sum(r['n_scored'] for r in on_disk['pieces'])
    assert abs(c['nll_mean'] - sum(r['nll_sum'] for r in on_disk['pieces']) / c['n_scored']) < 1e-9


def test_main_refuses_bad_arguments(tmp_path):
    from emo_disentanger_amd import scoring
    base = ['-m', 'gpt2', '-c', 'conf.yaml', '-r', 'functional', '--params', 'ckpt.pt']
    for extra in ([], ['--split', 'val', '--files', 'a.txt'], ['--split', 'test'], ['--files']):
        with pytest.raises(SystemExit):
            scoring.main(base + extra)
    with pytest.raises(SystemExit):
        scoring.main(['-m', 'lstm', '-c', 'conf.yaml', '-r', 'functional', '--params', 'ckpt.pt', '--files', 'a.txt'])
    with pytest.raises(SystemExit):
        scoring.main(base + ['--files', 'a.txt', '--batch', '0'])
    with pytest.raises(ValueError):
        scoring.score_tokens(None, None, None, want=('logprob', 'perplexity'))


def test_best_of_picks_the_lowest_score_first_on_ties():
    from emo_disentanger_amd import scoring
    nan = float('nan')
    assert scoring.best_of([2.0, 1.5, 1.7]) == 1
    assert scoring.best_of([1.5, 1.5, 1.5]) == 0
    assert scoring.best_of([2.0, 1.5, 1.5]) == 1
    assert scoring.best_of([nan, 3.0, 2.5]) == 2
    assert scoring.best_of([nan, nan]) == 0
    assert scoring.best_of([RuntimeError('x'), 4.0, nan]) == 1


def test_candidate_scores_keep_failed_candidates_in_place():
    from emo_disentanger_amd import scoring
    e2i, _ = _vocab()
    cands = [list(_piece(e2i, 2, seed=1, eos=False)[2]), RuntimeError('table exhausted'), list(_piece(e2i, 3, seed=2, eos=False)[2])]
    model = torch.nn.Linear(1, 1)
    model.n_token = len(e2i) + 1
    calls = []
    nll = scoring.candidate_scores(model, e2i, cands, max_len=500, batch=4, scorer=_stub_scorer(calls))
    assert len(nll) == 3 and math.isnan(nll[1]) and len(calls) == 1 and calls[0][0][0] == 2
    for i in (0, 2):
        tgt = scoring.targets_of(cands[i], e2i)[1]
        kept = tgt[tgt != len(e2i)]
        assert abs(nll[i] - float((0.5 + 0.01 * kept).mean())) < 1e-5
    assert scoring.best_of(nll) in (0, 2)
