"""CPU: the best-of tail that generate_lead_sheets and generate_accompaniments share (scoring.picks_of, generation_result, best_of_plan,
eval_mode), on plain lists, and both generators on fake loop classes: the same flags give the same-shaped tuple.  And what gen_loop gives
both generators around their loops: the request plan (plan_generation), the result tail (finish_generation) and the walk of the kept-bar
check (check_kept_bars)."""
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


# ------------------------------------------------------------------------------------------------ the request plan and the result tail
def _guided_plan(**kw):
    """3 inputs, inputs 1 and 2 guided, on plain lists: per-input entries are tagged by the input they belong to."""
    from emo_disentanger_amd import gen_loop
    i2e = {0: 'Emotion_None', 1: 'Emotion_Q1'}
    primers = [[1, 10], [1, 11], [1, 12]]
    guide = gen_loop.guidance_plan('t', [None, 2.0, 0.5], None, {'Emotion_None': 0}, i2e, primers)
    plan = gen_loop.plan_generation('t', 3, 40, None, kw.pop('keep', None), guide, dict(lead_sheets=['L0', 'L1', 'L2'], primers=primers,
                                                                                        max_events=[10, 20, 30]), **kw)
    return guide, plan


def test_plan_generation_puts_followers_behind_the_leaders_and_repeats_in_candidate_order():
    keep = [[[5]], None, [None, [6]]]
    guide, plan = _guided_plan(keep=keep, best_of=2, temp=[1.0, 1.1, 1.2], banned=[None, [7], [8]])
    order = [0, 0, 1, 1, 2, 2] + [1, 1, 2, 2]                        # leaders, candidate c of input i at i * 2 + c, then the followers alike
    assert plan.rows['lead_sheets'] == ['L%d' % i for i in order] and plan.rows['max_events'] == [10 * (i + 1) for i in order]
    assert plan.rows['primers'][:6] == [[1, 10 + i] for i in order[:6]]
    assert plan.rows['primers'][6:] == [[0, 10 + i] for i in order[6:]]                          # a follower's own primer: the unconditioned token
    assert plan.keep == [keep[i] for i in order] and plan.loop_kw['keep'] is plan.keep
    assert list(plan.rows) == ['lead_sheets', 'primers', 'max_events']                           # the order the caller gave: it may pass them positionally
    ctl = plan.controls
    assert ctl.n == 10 and (plan.best_of, plan.by_draws, plan.want_scores, plan.slots) == (2, False, False, None)
    for k in range(4):                                                                           # row n_in * 2 + k is paired with its leader
        g, c = 6 + k, order[6 + k] * 2 + k % 2
        assert ctl.guide_cond[g] == ctl.guide_cond[c] == c and ctl.guide_uncond[g] == ctl.guide_uncond[c] == g
        assert ctl.guide_scale[g] == ctl.guide_scale[c] == [0.0, 2.0, 0.5][order[6 + k]]
        assert (ctl.bans[g], ctl.temp_at(g)) == (ctl.bans[c], ctl.temp_at(c))
    assert ctl.guide_cond[:2] == [-1, -1] and ctl.followers() == [6, 7, 8, 9]
    assert plan.loop_kw['guidance'] == ctl.guide_arg and plan.loop_kw['temp'] == [[1.0, 1.1, 1.2][i] for i in order]
    assert plan.loop_kw['banned'] == [[None, (7,), (8,)][i] for i in order]


def test_plan_generation_leaves_unused_keywords_out_and_refuses_in_one_place():
    from emo_disentanger_amd import gen_loop
    rows = dict(primers=[[1], [2]])
    plan = gen_loop.plan_generation('t', 2, 40, None, None, None, rows, slots='3')
    assert set(plan.loop_kw) == {'temp', 'top_p', 'banned'} and plan.keep is None and plan.slots == 3
    assert plan.loop_kw == dict(temp=1.2, top_p=0.9, banned=[None, None]) and plan.rows == rows
    plan = gen_loop.plan_generation('t', 2, 40, None, [None, [[4]]], None, rows, best_of=2, best_by='draws', top_k=5)
    assert set(plan.loop_kw) == {'temp', 'top_p', 'banned', 'soft', 'keep'} and (plan.by_draws, plan.want_scores) == (True, True)
    assert plan.loop_kw['soft'] == dict(bias=None, top_k=[5] * 4, min_p=None) and plan.keep == [None, None, [[4]], [[4]]]
    guide, plan = _guided_plan()
    assert set(plan.loop_kw) == {'temp', 'top_p', 'banned', 'guidance'}
    with pytest.raises(ValueError, match='t: guidance runs in the lock-step batch: slots= is not available with it'):
        _guided_plan(slots=2)
    for bad in ('x', [1]):
        with pytest.raises(ValueError, match='slots must be None or a count of at least 1'):
            gen_loop.plan_generation('t', 2, 40, None, None, None, rows, slots=bad)
    with pytest.raises(ValueError, match=r'slots must be at least 1 \(got 0\)'):
        gen_loop.plan_generation('t', 2, 40, None, None, None, rows, slots=0)


def test_both_generators_refuse_a_slots_value_that_is_no_count_alike():
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    for bad in ('x', [2]):
        with pytest.raises(ValueError, match='slots must be None or a count of at least 1'):
            s1.generate_lead_sheets(_fake_model(False), {}, {}, [['Emotion_Q1']], slots=bad)
        with pytest.raises(ValueError, match='slots must be None or a count of at least 1'):
            inf.generate_accompaniments(_fake_model(False), {}, {}, [[[1]]], [[0]], slots=bad)


def test_finish_generation_leaves_a_broken_pair_as_an_error_that_never_wins_a_pick():
    import time
    from emo_disentanger_amd import gen_loop
    from emo_disentanger_amd._lib import EmoError
    guide, plan = _guided_plan(best_of=2, best_by='forward', return_scores=True)
    # rows: leaders [0 0 1 1 2 2], followers [1 1 2 2].  Candidate 0 of input 1 parts from its follower at token 2; every other pair holds
    res = [[1, 3], [1, 4], [1, 5, 9], [1, 6], [1, 7], [1, 8]] + [[0, 5, 2], [0, 6], [0, 7], [0, 8]]
    sc = [{'logp': np.array([NAN, -0.5 - j])} for j in range(10)]
    seen = []

    def forward(cands):                                              # the broken candidate would be the likeliest, were it scored
        seen.append(list(cands))
        return [NAN if isinstance(c, Exception) else float(j) for j, c in enumerate(cands)]

    got, secs, picks, scores = gen_loop.finish_generation(res, sc, [1] * 10, plan, guide, forward, time.time())
    assert len(seen) == 1 and len(seen[0]) == 6                      # the followers are gone before the ranking
    assert isinstance(seen[0][2], EmoError) and 'stream 2 and its unconditioned follower 6 left lock-step: the ids part at token 2' in str(seen[0][2])
    assert str(seen[0][2]).startswith('t: ')
    assert [p['chosen'] for p in picks] == [0, 1, 0] and got == [[1, 3], [1, 6], [1, 7]]
    assert isinstance(picks[1]['candidates'][0], EmoError) and picks[1]['scores'][0] is None
    assert 'logp_uncond' not in scores[0] and scores[1]['logp_uncond'] is sc[7]['logp'] and secs >= 0.0     # (the follower's row)
    # ranked by the recorded draws: the error's scores are None, NaN, and never win either
    guide, plan = _guided_plan(best_of=2, best_by='draws')
    got, _, picks = gen_loop.finish_generation(res, [dict(s, rank=np.array([-1, 0])) for s in sc], [1] * 10, plan, guide, None, time.time())
    assert [p['chosen'] for p in picks] == [0, 1, 0] and picks[1]['nll_mean'][0] != picks[1]['nll_mean'][0]
    # status words that part break a pair whatever the ids say
    guide, plan = _guided_plan()
    out, _ = gen_loop.finish_generation([[1, 3], [1, 4], [1, 5], [0, 4], [0, 5]], None, [1, 1, 1, 2, 1], plan, guide, None, time.time())
    assert out[0] == [1, 3] and isinstance(out[1], EmoError) and 'status 1 against 2' in str(out[1]) and out[2] == [1, 5]


def test_each_shared_kept_bar_refusal_raises_once_per_stage_with_the_stages_noun():
    from emo_disentanger_amd import gen_loop, inference as inf, stage1_inference as s1
    e2i = {'Track_LeadSheet': 1, 'Track_Full': 2, 'EOS_None': 3, 'PAD_None': 4, 'Bar_None': 5}
    i2e = {i: e for e, i in e2i.items()}
    two = lambda keep: inf.check_keep('two', keep, [[[7]], [[8], [9]]], 40, e2i)                 # noqa: E731
    one = lambda keep, pb=None: s1.check_keep('one', keep, 2, 40, i2e, pb)                      # noqa: E731
    for keep, text in (([None], 'keep has 1 entries for 2 %s'), ([[7], None], r'keep\[0\]\[0\] is neither None nor a sequence of token ids'),
                       ([[['x']], None], r'keep\[0\]\[0\] is neither None nor a sequence of token ids'),
                       ([None, [None, [40]]], r'keep\[1\]\[1\] holds token id 40 outside \[0, 40\)'),
                       ([None, [[-1]]], r'keep\[1\]\[0\] holds token id -1 outside \[0, 40\)')):
        with pytest.raises(ValueError, match='two: ' + text.replace('%s', 'inputs')):
            two(keep)
        with pytest.raises(ValueError, match='one: ' + text.replace('%s', 'primers')):
            one(keep)
    for check in (two, one):                                         # nothing kept is None; what is kept comes back as ints, bar for bar
        assert check(None) is None and check([None, None]) is None and check([[None], [None, None]]) is None
        assert check([[np.array([6, 7])], (None, (8,))]) == [[[6, 7]], [None, [8]]]
    # each stage's own rule, through the walker's refuse(i, j, ids)
    with pytest.raises(ValueError, match=r'two: keep\[1\]\[0\] holds Track_Full, which the grammar writes itself around a bar'):
        two([None, [[6, 2]]])
    with pytest.raises(ValueError, match=r'two: keep\[0\] has 2 bars, its lead sheet 1'):
        two([[None, None], None])
    with pytest.raises(ValueError, match=r'one: keep\[1\]\[0\] holds Bar_None, which the grammar writes or rejects itself'):
        one([None, [[6, 5]]])
    with pytest.raises(ValueError, match=r"one: keep\[1\]\[0\] lies under prompt_bars = 1: a primer's own bars are never kept"):
        one([None, [[6]]], [0, 1])
    with pytest.raises(ValueError, match='one: prompt_bars: 3 values for 2 primers'):
        one([None, [[6]]], [0, 1, 2])
    seen = []
    assert gen_loop.check_kept_bars('w', [[None, [1, 2]], None, [[]]], 3, 9, 'things', lambda i, j, ids: seen.append((i, j, ids))) == [[None, [1, 2]], None, [[]]]
    assert seen == [(0, 1, [1, 2]), (2, 0, [])]
