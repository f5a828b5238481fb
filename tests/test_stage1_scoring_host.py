"""Host logic of the stage-1 lead-sheet scoring (no GPU): target / mask construction, the best-of-N pick, the primer_outside_window flag and the
--stage 1 command line with stand-ins for the model and the scorer."""
import json
import pickle

import pytest
import torch

PAD = 9


def test_targets_are_the_next_token_between_the_primer_and_the_end_of_each_row():
    from emo_disentanger_amd import scoring
    tok = torch.tensor([[1, 2, 3, 4, 5, 6],            # length 6, primer 1: positions 0 .. 4 predict tokens 1 .. 5
                        [1, 2, 3, 4, PAD, PAD],        # length 4, primer 3: positions 2 predicts token 3; 0, 1 are inside the primer
                        [1, PAD, 3, 4, 5, PAD],        # length 5, primer 1: a PAD inside the row is no target
                        [7, PAD, PAD, PAD, PAD, PAD]])  # length 1: nothing to predict
    tgt = scoring.lead_sheet_targets(tok, [6, 4, 5, 1], [1, 3, 1, 1], PAD)
    assert tgt.tolist() == [[2, 3, 4, 5, 6, PAD],
                            [PAD, PAD, 4, PAD, PAD, PAD],
                            [PAD, 3, 4, 5, PAD, PAD],
                            [PAD] * 6]
    # one primer length for every row; a primer as long as the row leaves nothing
    assert scoring.lead_sheet_targets(tok[:2], [6, 4], 4, PAD).tolist() == [[PAD, PAD, PAD, 5, 6, PAD], [PAD] * 6]
    # whatever sits past a row's length is never a target, PAD or not
    assert scoring.lead_sheet_targets(torch.tensor([[1, 2, 3, 4, 5, 6]]), [3], 1, PAD).tolist() == [[2, 3, PAD, PAD, PAD, PAD]]


def test_batches_pad_each_group_to_its_longest_row():
    from emo_disentanger_amd import scoring
    lists = [[1, 2, 3], [4, 5, 6, 7, 8], [1, 2]]
    got = list(scoring.lead_sheet_batches(lists, [1, 2, 1], 2, PAD, ids=['a', 'b', 'c']))
    assert [b['piece_id'] for b in got] == [['a', 'b'], ['c']]
    assert got[0]['tokens'].tolist() == [[1, 2, 3, PAD, PAD], [4, 5, 6, 7, 8]] and got[1]['tokens'].tolist() == [[1, 2]]
    assert got[0]['length'] == [3, 5] and got[0]['primer_len'] == [1, 2] and got[1]['primer_len'] == [1]


class _StubModel(torch.nn.Module):
    """What score_lead_sheets reads from a model: its device, its PAD (n_token - 1) and its memory length."""

    def __init__(self, n_token=PAD + 1, mem_len=4):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.n_token, self.dec_mem_len = n_token, mem_len


def _stub_scorer(calls):
    """logprob = -(target id) / 10, rank = target id % 7, entropy = 0.5, by the module's own target rule."""
    from emo_disentanger_amd import scoring

    def scorer(model, tokens, lengths, primer_len, window=None):
        calls.append((tuple(tokens.shape), list(lengths), list(primer_len), window))
        tgt = scoring.lead_sheet_targets(tokens, lengths, primer_len, model.n_token - 1)
        mask = tgt != model.n_token - 1
        return scoring.TokenScores(torch.where(mask, -tgt.float() / 10, torch.zeros(())), torch.where(mask, tgt % 7, torch.full_like(tgt, -1)).int(),
                                   torch.full(tgt.shape, 0.5), mask)
    return scorer


def test_records_carry_primer_outside_window_exactly_past_window_plus_one():
    from emo_disentanger_amd import scoring
    calls = []
    lists = [list(range(1, 9))] * 5
    primers = [1, 4, 5, 6, 8]
    recs = scoring.score_lead_sheets(_StubModel(mem_len=4), lists, primers, batch=2, scorer=_stub_scorer(calls))
    assert [r['primer_outside_window'] for r in recs] == [False, False, False, True, True]       # window 4: a primer of up to 5 tokens is inside
    assert [c[3] for c in calls] == [4, 4, 4] and [c[0][0] for c in calls] == [2, 2, 1]
    recs = scoring.score_lead_sheets(_StubModel(mem_len=4), lists, primers, batch=8, window=5, scorer=_stub_scorer(calls))
    assert [r['primer_outside_window'] for r in recs] == [False, False, False, False, True] and calls[-1][3] == 5
    keys = set(scoring.piece_record('x', 1, 1, 1.0, 1, 1, 1.0))
    assert all(set(r) == keys | {'primer_outside_window'} for r in recs)
    r = recs[1]                                                            # primer 4 of 8 tokens: targets 5, 6, 7, 8
    assert r['n_tokens'] == 8 and r['n_scored'] == 4 and abs(r['nll_sum'] - 2.6) < 1e-6 and abs(r['entropy_mean'] - 0.5) < 1e-9
    assert r['top1'] == 0.25 and r['top5'] == 0.5                          # ranks 5, 6, 0, 1
    assert recs[4]['n_scored'] == 0 and recs[4]['nll_mean'] != recs[4]['nll_mean']


def test_candidate_scores_keep_failed_candidates_in_place():
    from emo_disentanger_amd import scoring
    cands = [[1, 2, 3], None, ValueError('key generation failed'), [1, 5, 6, 7]]
    got = scoring.lead_sheet_candidate_scores(_StubModel(), cands, [1, 1, 1, 1], scorer=_stub_scorer([]))
    assert abs(got[0] - 0.25) < 1e-6 and got[1] != got[1] and got[2] != got[2] and abs(got[3] - 0.6) < 1e-6


def test_best_of_ties_go_to_the_lowest_index_and_a_failed_candidate_never_wins():
    from emo_disentanger_amd import stage1_inference as s1
    nan = float('nan')
    table = {'a': 2.0, 'b': 1.0, 'c': 1.0, 'd': 3.0, 'e': 0.5}
    cands = [['a'], ['b'], ['c'],                      # a tie between candidates 1 and 2 -> 1
             None, ['d'], ValueError('x'),             # the only one that finished wins, whatever its score
             None, ValueError('y'), None,              # nothing finished: candidate 0 (a failure) is handed back
             ['e'], ['b'], ['a']]
    seen = {}

    def scorer(model, candidates, primer_lens):
        seen['primer_lens'] = list(primer_lens)
        return [nan if not isinstance(c, list) else table[c[0]] for c in candidates]
    picks = s1.pick_best(None, cands, [1] * 12, 3, scorer=scorer)
    assert [p['chosen'] for p in picks] == [1, 1, 0, 0]
    assert picks[1]['candidates'][1] == ['d'] and picks[2]['candidates'][picks[2]['chosen']] is None
    assert picks[0]['nll_mean'] == [2.0, 1.0, 1.0] and len(picks) == 4 and seen['primer_lens'] == [1] * 12
    with pytest.raises(ValueError):
        s1.generate_lead_sheets(None, {}, {}, [['Emotion_Q1']], best_of=0)


def _stage1_workspace(tmp_path):
    events = ['Emotion_Q1', 'Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Note_Degree_1', 'Note_Duration_2', 'Chord_I_M', 'EOS_None']
    e2i = {e: i for i, e in enumerate(events)}
    with open(tmp_path / 'dictionary.pkl', 'wb') as fh:
        pickle.dump((e2i, {i: e for e, i in e2i.items()}), fh)
    (tmp_path / 'conf.yaml').write_text(
        "data:\n  vocab_path: %s\nmodel:\n  d_word_embed: 64\n  pre_lnorm: True\n  decoder:\n    n_layer: 2\n    n_head: 4\n    d_model: 64\n    d_ff: 128\n"
        "    dropout: 0.1\n    mem_len: 0\n    tgt_len: 6\n" % (tmp_path / 'dictionary.pkl'))
    files = []
    for name, body in (('samp_00_Q1_roman.txt', ['Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M']),             # as stage1_inference.main writes them: no tag
                       ('samp_01_Positive.txt', ['Bar_None', 'Beat_0', 'Note_Degree_1', 'Note_Duration_2', 'Bar_None']),
                       ('tagged.txt', ['Emotion_Q1', 'Key_C', 'Bar_None'])):
        (tmp_path / name).write_text('\n'.join(body) + '\n')
        files.append(str(tmp_path / name))
    return e2i, files


def test_stage1_command_line_with_a_stub_loader(tmp_path):
    from emo_disentanger_amd import scoring
    e2i, files = _stage1_workspace(tmp_path)
    assert scoring.read_lead_sheet_file(files[0], e2i) == ([e2i[e] for e in ('Emotion_Q1', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M')], 1)
    assert scoring.read_lead_sheet_file(files[2], e2i)[0] == [e2i[e] for e in ('Emotion_Q1', 'Key_C', 'Bar_None')]
    seen, calls = {}, []

    def load_model(args, conf, n_token):
        seen.update(n_token=n_token, dtype=args.dtype, stage=args.stage)
        return _StubModel(n_token=n_token, mem_len=conf['model']['decoder']['tgt_len'])
    out = tmp_path / 'scores.json'
    res = scoring.main(['--stage', '1', '-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '--params', 'ckpt.pt', '--dtype', 'fp32', '--batch', '2',
                        '--files'] + files + ['-o', str(out)], scorer=_stub_scorer(calls), load_model=load_model)
    assert seen == {'n_token': len(e2i) + 1, 'dtype': 'fp32', 'stage': 1}             # the stage-1 vocabulary: PAD appended after the dictionary
    assert [c[0] for c in calls] == [(2, 6), (1, 3)] and all(c[3] == 6 for c in calls) and calls[0][2] == [1, 1]
    on_disk = json.load(open(out))
    assert [p['id'] for p in on_disk['pieces']] == ['samp_00_Q1_roman', 'samp_01_Positive', 'tagged']
    assert [p['n_tokens'] for p in on_disk['pieces']] == [5, 6, 3] and [p['n_scored'] for p in on_disk['pieces']] == [4, 5, 2]
    assert all(p['primer_outside_window'] is False for p in on_disk['pieces'])
    assert on_disk['model'] == {'type': 'stage1_txl', 'params': 'ckpt.pt', 'dtype': 'fp32', 'window': 6}
    assert on_disk['corpus']['n_pieces'] == 3 and on_disk['corpus']['n_scored'] == 11 and res['corpus'] == on_disk['corpus']
    # --window overrides the configuration's
    scoring.main(['--stage', '1', '-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '--params', 'ckpt.pt', '--window', '3', '--files', files[0], '-o', str(out)],
                 scorer=_stub_scorer(calls), load_model=load_model)
    assert calls[-1][3] == 3 and json.load(open(out))['model']['window'] == 3


def test_stage1_command_line_refuses_what_it_cannot_serve(tmp_path):
    from emo_disentanger_amd import scoring, stage1_inference as s1
    _, files = _stage1_workspace(tmp_path)
    base = ['-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '--params', 'ckpt.pt']
    for argv in (['--stage', '1'] + base + ['--split', 'val'],                       # stage 1 scores files
                 ['--stage', '1'] + base + ['--files', files[0], '--window', '0'],
                 ['--stage', '3'] + base + ['--files', files[0]],
                 base + ['--files', files[0]],                                       # stage 2 needs -m
                 ['-m', 'gpt2'] + base + ['--files', files[0], '--window', '4']):     # --window is a stage-1 option
        with pytest.raises(SystemExit):
            scoring.main(argv, load_model=lambda *a: _StubModel())
    (tmp_path / 'noname.txt').write_text('Bar_None\n')
    with pytest.raises(ValueError, match='no Emotion'):
        scoring.main(['--stage', '1'] + base + ['--files', str(tmp_path / 'noname.txt')], load_model=lambda *a: _StubModel())
    # the generator's side of the feature: --best-of is parsed, and refused with the host-exact loop
    args = s1.parse_args(['-c', 'c.yaml', '-r', 'functional', '-m', 'lead_sheet', '--best-of', '4'])
    assert args.best_of == 4 and s1.parse_args(['-c', 'c.yaml', '-r', 'functional', '-m', 'lead_sheet']).best_of == 1
    for bad in (['--best-of', '0'], ['--best-of', '2', '--exact']):
        with pytest.raises(SystemExit):
            s1.parse_args(['-c', 'c.yaml', '-r', 'functional', '-m', 'lead_sheet'] + bad)
