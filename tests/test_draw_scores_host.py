"""CPU: the host side of the per-draw scores — the three fields of the GrammarStep mirror, the entry's refusals with them set, scoring.draw_record /
draw_scores_mean on hand-made arrays, best_by validation, and the --scores / --best-by arguments of the two generation command lines."""
import ctypes
import json
import math

import numpy as np
import pytest

NAN = float('nan')


def test_the_grammar_step_mirror_has_the_three_trailing_fields():
    from emo_disentanger_amd import _lib
    names = [f[0] for f in _lib.GrammarStep._fields_]
    assert names[-3:] == ['tok_logp', 'tok_rank', 'tok_entropy']
    assert all(f[1] is _lib.c_p for f in _lib.GrammarStep._fields_[-3:])
    assert _lib.lib.emo_grammar_step_size() == ctypes.sizeof(_lib.GrammarStep)
    a = _lib.GrammarStep()
    assert a.tok_logp is None and a.tok_rank is None and a.tok_entropy is None        # off by default


def _block(kind, **kw):
    """A block that passes every host check of `kind`, the three outputs set (fake addresses: no refusal below reaches a launch)."""
    from emo_disentanger_amd import _lib
    a = _lib.GrammarStep()
    for name, ctype in _lib.GrammarStep._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.kind, a.n_rows, a.n_token, a.n_u, a.ld_u, a.ld_seq, a.max_len, a.window = kind, 3, 327, 8, 3, 64, 32, 32
    a.temperature, a.top_p, a.key_temperature, a.key_top_p = 1.2, 0.9, 1.1, 0.97
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('kind, name', [(0, 'txl'), (1, 'acc'), (2, 'acc_window')])
def test_the_entry_still_refuses_bad_blocks_by_kind_with_the_outputs_set(kind, name):
    from emo_disentanger_amd import _lib
    for kw, what in ((dict(n_token=2000), 'V must be <= 1024 (got 2000)'), (dict(temperature=0.0), 'must be > 0'), (dict(n_u=0), 'bad sizes'),
                     (dict(seq=None), 'null pointer')):
        a = _block(kind, **kw)
        assert a.tok_logp == 0x1000 and a.tok_rank == 0x1000 and a.tok_entropy == 0x1000
        assert _lib.lib.emo_grammar_step(ctypes.byref(a), None) == -1
        msg = _lib.lib.emo_last_error().decode()
        assert msg.startswith('emo_grammar_step[%s]: ' % name) and what in msg, msg


def test_draw_record_skips_the_sentinels_and_matches_piece_record():
    from emo_disentanger_amd import scoring
    ids = [9, 4, 7, 7, 2, 5, 1]
    logp = np.array([NAN, NAN, -0.5, -2.0, NAN, -0.25, -3.0], np.float32)
    rank = np.array([-1, -1, 0, 3, -1, 0, 7], np.int32)
    ent = np.array([NAN, NAN, 1.0, 2.0, NAN, 0.5, 2.5], np.float32)
    rec = scoring.draw_record(ids, logp, rank, ent, pid='x')
    want = scoring.piece_record('x', 7, 4, 0.5 + 2.0 + 0.25 + 3.0, 2, 3, 1.0 + 2.0 + 0.5 + 2.5)
    assert rec == want
    assert rec['n_scored'] == 4 and rec['nll_mean'] == pytest.approx(5.75 / 4) and rec['ppl'] == pytest.approx(math.exp(5.75 / 4))
    assert rec['top1'] == 0.5 and rec['top5'] == 0.75 and rec['entropy_mean'] == 1.5
    # nothing drawn: a record of NaNs, as piece_record gives for nothing scored
    none = scoring.draw_record([1, 2], [NAN, NAN], [-1, -1], [NAN, NAN])
    assert none['n_scored'] == 0 and none['n_tokens'] == 2 and none['nll_mean'] != none['nll_mean']
    with pytest.raises(ValueError):
        scoring.draw_record(ids, logp[:-1], rank, ent)


def test_a_candidate_without_draws_scores_nan_and_never_wins():
    from emo_disentanger_amd import scoring
    sc = lambda lp, rk: {'logp': np.array(lp, np.float32), 'rank': np.array(rk, np.int32), 'entropy': np.zeros(len(lp), np.float32)}   # noqa: E731
    cands = [None, sc([NAN, NAN], [-1, -1]), sc([NAN, -2.0, -4.0], [-1, 0, 5]), sc([NAN, -1.0], [-1, 2])]
    means = scoring.draw_scores_mean(cands)
    assert means[0] != means[0] and means[1] != means[1] and means[2:] == [3.0, 1.0]
    assert scoring.best_of(means) == 3
    assert scoring.best_of(means[:3]) == 2                        # the only scored one, although it comes last
    assert scoring.best_of(means[:2]) == 0                        # nothing scored: the first, as with 'forward'


def test_best_by_is_validated_before_anything_runs():
    from emo_disentanger_amd import inference as inf, scoring, stage1_inference as s1
    assert scoring.BEST_BY == ('forward', 'draws')
    for ok in scoring.BEST_BY:
        scoring.check_best_by(ok)

    class NoModel:
        n_token = 10
    with pytest.raises(ValueError, match="best_by must be one of 'forward', 'draws'"):
        s1.generate_lead_sheets(NoModel(), {}, {}, [['Emotion_Q1']], best_of=2, best_by='sum')
    with pytest.raises(ValueError, match="best_by must be one of 'forward', 'draws'"):
        inf.generate_accompaniments(NoModel(), {}, {}, [[[1]]], [[0]], best_of=2, best_by='sum')


S1 = ['-c', 'c.yaml', '-r', 'functional', '-m', 'lead_sheet']
S2 = ['-m', 'gpt2', '-c', 'c.yaml', '-r', 'functional', '-i', 'w.pt', '-o', 'out']


def test_stage1_command_line_takes_scores_and_best_by(capsys):
    from emo_disentanger_amd import stage1_inference as s1
    a = s1.parse_args(S1)
    assert a.best_by == 'forward' and a.scores is None
    a = s1.parse_args(S1 + ['--best-of', '4', '--best-by', 'draws', '--scores', 's.json'])
    assert (a.best_of, a.best_by, a.scores) == (4, 'draws', 's.json')
    for bad in (['--best-by', 'draws'], ['--scores', 's.json', '--exact'], ['--best-of', '2', '--best-by', 'sum']):
        with pytest.raises(SystemExit):
            s1.parse_args(S1 + bad)
    capsys.readouterr()


def test_stage2_command_line_takes_scores_and_best_by(capsys):
    from emo_disentanger_amd import inference as inf
    a = inf.parse_args(S2)
    assert a.best_by == 'forward' and a.scores is None and not a.device
    a = inf.parse_args(S2 + ['--device', '--best-of', '2', '--best-by', 'draws', '--scores', 's.json', '--window', 'device'])
    assert (a.best_of, a.best_by, a.scores, a.window) == (2, 'draws', 's.json', 'device')
    for bad in (['--scores', 's.json'], ['--device', '--best-by', 'draws'], ['--device', '--best-of', '2', '--best-by', 'sum']):
        with pytest.raises(SystemExit):
            inf.parse_args(S2 + bad)
    assert '--scores needs --device' in capsys.readouterr().err.split('usage')[1]


def test_the_scores_file_holds_a_record_and_the_token_rows_per_piece(tmp_path):
    from emo_disentanger_amd import scoring
    sc = {'logp': np.array([NAN, -1.0, -3.0], np.float32), 'rank': np.array([-1, 0, 6], np.int32), 'entropy': np.array([NAN, 1.0, 2.0], np.float32)}
    empty = {'logp': np.array([NAN], np.float32), 'rank': np.array([-1], np.int32), 'entropy': np.array([NAN], np.float32)}
    pieces = scoring.draw_pieces(['a', 'b', 'c', 'd'], [[5, 6, 7], None, ValueError('key'), [5]], [sc, None, None, empty])
    path = tmp_path / 's.json'
    scoring.write_draw_scores(str(path), pieces)
    got = json.loads(path.read_text())                             # (strict JSON: no NaN in the file)
    a, b, c, d = got['pieces']
    assert a['id'] == 'a' and a['n_scored'] == 2 and a['nll_mean'] == 2.0 and a['top1'] == 0.5
    assert a['tokens'] == {'ids': [5, 6, 7], 'rank': [-1, 0, 6], 'logp': [None, -1.0, -3.0], 'entropy': [None, 1.0, 2.0]}
    assert 'stuck' in b['failed'] and c['failed'] == 'key'
    assert d['n_scored'] == 0 and d['nll_mean'] is None
    assert got['corpus']['n_scored'] == 2 and got['corpus']['n_pieces'] == 2 and got['corpus']['nll_mean'] == 2.0
