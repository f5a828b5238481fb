"""CPU: the best-of tail that generate_lead_sheets and generate_accompaniments share (scoring.picks_of, generation_result, best_of_plan,
eval_mode), on plain lists, and both generators on fake loop classes: the same flags give the same-shaped tuple."""
from types import SimpleNamespace

import numpy as np
import pytest

NAN = float('nan')


def test_picks_of_follows_best_of_on_nan_all_nan_and_ties():
    from emo_disentanger_amd import scoring
    results = [[1], [2], ValueError('x'), None, [5], [6]]
    nll = [NAN, 0.7, NAN, NAN, 0.25, 0.25]
    picks = scoring.picks_of(results, nll, 2)
    assert [p['chosen'] for p in picks] == [1, 0, 0]                 # a NaN never wins; all NaN: what best_of gives (0); a tie: the lowest index
    assert [p['chosen'] for p in picks] == [scoring.best_of(nll[i:i + 2]) for i in (0, 2, 4)]
    assert [p['candidates'] for p in picks] == [results[0:2], results[2:4], results[4:6]]
    assert picks[0]['nll_mean'][1] == 0.7 and picks[2]['nll_mean'] == [0.25, 0.25]
    assert all(set(p) == {'chosen', 'nll_mean', 'candidates'} for p in picks)
    scores = ['s%d' % i for i in range(6)]
    with_scores = scoring.picks_of(results, nll, 2, scores)
    assert [p['scores'] for p in with_scores] == [['s0', 's1'], ['s2', 's3'], ['s4', 's5']]
    assert [p['chosen'] for p in with_scores] == [1, 0, 0]


@pytest.mark.parametrize('best_of', [1, 2])
@pytest.mark.parametrize('return_scores', [False, True])
def test_generation_result_is_the_tuple_the_generators_document(best_of, return_scores):
    from emo_disentanger_amd import scoring
    results, scores = [[1], [2], [3], [4]], ['a', 'b', 'c', 'd']
    picks = scoring.picks_of(results, [0.5, 0.1, 0.2, 0.9], 2, scores if return_scores else None) if best_of > 1 else None
    got = scoring.generation_result(results, 1.5, scores, picks, return_scores)
    if best_of == 1:
        assert got == (([[1], [2], [3], [4]], 1.5, ['a', 'b', 'c', 'd']) if return_scores else ([[1], [2], [3], [4]], 1.5))
    else:                                                            # (the chosen candidates, seconds, picks[, the chosen candidates' scores])
        assert got[:3] == ([[2], [3]], 1.5, picks) and len(got) == (4 if return_scores else 3)
        if return_scores:
            assert got[3] == ['b', 'c']


def test_best_of_plan_checks_and_repeats_in_candidate_order():
    from emo_disentanger_amd import scoring
    with pytest.raises(ValueError, match='best_of must be at least 1'):
        scoring.best_of_plan(0, 'forward', False)
    with pytest.raises(ValueError, match='best_by must be one of'):
        scoring.best_of_plan(2, 'likelihood', False)
    n, by_draws, want, a, b = scoring.best_of_plan(3, 'forward', False, ['x', 'y'], [[1], [2]])
    assert (n, by_draws, want) == (3, False, False)
    assert a == ['x', 'x', 'x', 'y', 'y', 'y'] and b == [[1], [1], [1], [2], [2], [2]]          # candidate c of input i is entry i * N + c
    assert all(a[i * 3 + c] == 'xy'[i] for i in range(2) for c in range(3))
    assert scoring.best_of_plan(2, 'draws', False)[:3] == (2, True, True)                     # ranking by draws needs them recorded
    assert scoring.best_of_plan(1, 'draws', False)[:3] == (1, False, False)                   # nothing to rank
    assert scoring.best_of_plan('2', 'forward', True, [7])[1:] == (False, True, [7, 7])


def _fake_model(training):
    m = SimpleNamespace(training=training, calls=[], n_token=40)
    m.eval = lambda: m.calls.append('eval')
    m.train = lambda mode=True: m.calls.append(('train', mode))
    return m


def test_eval_mode_restores_the_mode_also_when_the_block_raises():
    from emo_disentanger_amd import scoring
    for training in (True, False):
        m = _fake_model(training)
        with scoring.eval_mode(m):
            assert m.calls == ['eval']
        assert m.calls == ['eval', ('train', training)]
        m = _fake_model(training)
        with pytest.raises(KeyError):
            with scoring.eval_mode(m):
                raise KeyError('x')
        assert m.calls == ['eval', ('train', training)]


class _FakeLoop:
    """What the generators ask of a loop.  Candidate c of input i gets ids [i, c]; its recorded logp makes the LAST candidate the likeliest by
    draws, the scoring forward (stubbed below) makes the FIRST one the likeliest."""
    bound = 48

    def __init__(self, model, e2i, i2e, *inputs, **kw):
        self.n, self.kw = len(inputs[0]), kw
        assert all(len(x) == self.n for x in inputs)                 # per-input lists were repeated alike: stage 1's per-primer max_events too
        assert not isinstance(kw['max_events'], list) or kw['max_events'] == [10 * (j // (self.n // 3) + 1) for j in range(self.n)]
        self.params = SimpleNamespace(cpu=lambda: SimpleNamespace(numpy=lambda: np.ones((self.n, 8), dtype=np.int32)))

    def run(self, use_graph=True):
        pass

    def results(self, *a, **kw):
        return [[j, j + 100] for j in range(self.n)]

    def scores(self, results=None):
        assert self.kw['scores']
        return [{'logp': np.array([NAN, -1.0 / (j + 1)]), 'rank': np.array([-1, 0]), 'entropy': np.array([NAN, 0.5])} for j in range(self.n)]


@pytest.mark.parametrize('best_of', [1, 2])
@pytest.mark.parametrize('return_scores', [False, True])
@pytest.mark.parametrize('best_by', ['forward', 'draws'])
def test_both_generators_return_the_same_shaped_tuple_for_the_same_flags(monkeypatch, best_of, return_scores, best_by):
    from emo_disentanger_amd import inference as inf, scoring, stage1_inference as s1
    monkeypatch.setattr(s1, 'LeadSheetLoop', _FakeLoop)
    monkeypatch.setattr(inf, 'AccompanimentLoop', _FakeLoop)
    forward = lambda n: [float(j % best_of) for j in range(n)]                                # noqa: E731  (candidate 0 the likeliest)
    monkeypatch.setattr(scoring, 'lead_sheet_candidate_scores', lambda model, cands, plens: forward(len(cands)))
    monkeypatch.setattr(scoring, 'candidate_scores', lambda model, e2i, cands, max_len: forward(len(cands)))
    flags = dict(best_of=best_of, best_by=best_by, return_scores=return_scores)
    m1, m2 = _fake_model(True), _fake_model(False)
    one = s1.generate_lead_sheets(m1, {}, {}, [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Q3']], max_events=[10, 20, 30], **flags)
    two = inf.generate_accompaniments(m2, {}, {}, [[[1]], [[2]], [[3]]], [[0], [0], [0]], **flags)
    assert m1.calls == ['eval', ('train', True)] and m2.calls == ['eval', ('train', False)]
    chosen = 0 if best_of == 1 or best_by == 'forward' else best_of - 1
    for got in (one, two):
        assert len(got) == 2 + (best_of > 1) + return_scores
        assert got[0] == [[i * best_of + chosen, i * best_of + chosen + 100] for i in range(3)] and got[1] >= 0.0
        if best_of > 1:
            picks = got[2]
            assert [p['chosen'] for p in picks] == [chosen] * 3 and all(('scores' in p) == return_scores for p in picks)
            assert [p['candidates'] for p in picks] == [[[2 * i, 2 * i + 100], [2 * i + 1, 2 * i + 101]] for i in range(3)]
        if return_scores:
            assert len(got[-1]) == 3 and all(set(sc) == {'logp', 'rank', 'entropy'} for sc in got[-1])
            assert [float(sc['logp'][1]) for sc in got[-1]] == [-1.0 / (i * best_of + chosen + 1) for i in range(3)]
    assert [type(x) for x in one] == [type(x) for x in two]
