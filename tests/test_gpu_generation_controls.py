"""GPU: the sampling controls through the device generation loops — generate_accompaniments / generate_lead_sheets (banned=, per-input temp /
top_p) on the small fp32 models of test_gpu_stage2_batch.py / test_gpu_stage1_batch.py: per-stream bans (the drawn tokens are told from the
given ones by the score tables), a batch against one-row runs, the queue against lock-step, best_of, the windowed phase on the device, the
hand-over to the host finish, and key forcing in stage 1."""
from collections import Counter

import numpy as np
import pytest
import torch

import test_gpu_stage1_batch as s1b
import test_gpu_stage2_batch as s2b

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def s2():
    """The tiny fp32 GPT-2 (rows of a batch do not touch each other), its vocabulary, and three lead sheets of 2-3 bars that open with the
    same bar under primers of one length: every prompt is the common prefix, in a batch as alone."""
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = s2b._vocab()
    lead = [list(b) for b in g['lead']]
    leads = [[lead[0], lead[1]], [lead[0], lead[2], lead[1]], [lead[0], lead[1], lead[2]]]
    primers = [[0, 4, 6], [1, 5, 6], [2, 4, 6]]
    return inf, s2b._tiny('gpt2', 'fp32'), e2i, i2e, leads, primers


KW = dict(max_events=60, skip_check=False, seed=3)


def drawn(ids, sc):
    """[(position, id)] of the tokens of a result that were drawn (the score tables hold a rank there), and the given ones"""
    d = [(c, t) for c, (t, r) in enumerate(zip(ids, sc['rank'])) if r >= 0]
    return d, [(c, t) for c, (t, r) in enumerate(zip(ids, sc['rank'])) if r < 0]


def favourites(results, scores, k=3, spare=()):
    """the k ids drawn most often in `results`: a ban on them is a ban that bites"""
    cnt = Counter(t for ids, sc in zip(results, scores) for _, t in drawn(ids, sc)[0] if t not in spare)
    return [t for t, _ in cnt.most_common(k)]


def test_per_stream_bans_hold_for_draws_and_for_nothing_else(s2):
    inf, model, e2i, i2e, leads, primers = s2
    base, _, sc0 = inf.generate_accompaniments(model, e2i, i2e, leads, primers, return_scores=True, **KW)
    spare = {e2i['Track_LeadSheet'], e2i['EOS_None']}
    # stream 0: its favourites and two ids its prompt holds (Tempo_110 in the primer, Note_Octave_4 in the lead-sheet bars); stream 2: its own
    ban0 = sorted(set(favourites(base[:1], sc0[:1], spare=spare)) | {e2i['Tempo_110'], e2i['Note_Octave_4']})
    ban2 = sorted(favourites(base[2:], sc0[2:], spare=spare))
    assert ban0 and ban2
    got, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, banned=[ban0, None, ban2], return_scores=True, **KW)
    assert got[1] == base[1]                                       # the unbanned stream: the run without `banned`
    assert got[0] != base[0] and got[2] != base[2]
    for i, ban in ((0, ban0), (2, ban2)):
        d, given = drawn(got[i], sc[i])
        assert len(d) >= 5 and not {t for _, t in d} & set(ban), (i, d)
    given0 = [t for _, t in drawn(got[0], sc[0])[1]]
    assert e2i['Tempo_110'] in given0 and e2i['Note_Octave_4'] in given0      # fed as they are, banned or not
    # one sequence of ids holds for every input
    every, _, sce = inf.generate_accompaniments(model, e2i, i2e, leads, primers, banned=ban2, return_scores=True, **KW)
    assert every[2] == got[2]
    assert all(not {t for _, t in drawn(ids, s)[0]} & set(ban2) for ids, s in zip(every, sce))


def _alone(inf, model, e2i, i2e, lead, primer, U_col, **kw):
    """One stream in a one-row loop, on the column of uniforms it has in the batch."""
    loop = inf.AccompanimentLoop(model, e2i, i2e, [lead], [primer], n_u=U_col.shape[0], **kw)
    loop.U.copy_(U_col.view(-1, 1))
    loop.run()
    return loop.results(e2i, i2e, kw['max_events'], kw['skip_check'], kw['seed'])[0]


def test_a_batch_with_per_input_parameters_equals_one_row_runs_with_the_scalars(s2):
    inf, model, e2i, i2e, leads, primers = s2
    temps, top_ps, ban = [0.8, 1.2, 1.7], [0.9, 0.97, 0.6], [None, [e2i['Beat_3'], e2i['Chord_I_M']], None]
    with torch.no_grad():
        big = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, temp=temps, top_p=top_ps, banned=ban, **KW)
        big.run()
        got = big.results(e2i, i2e, KW['max_events'], False, KW['seed'])
        assert sorted(big.control_tables) == ['mask_of', 'temp_of', 'tok_mask', 'top_p_of'] and big._gargs.n_masks == 1
        for i in range(3):
            one = _alone(inf, model, e2i, i2e, leads[i], primers[i], big.U[:, i], temp=temps[i], top_p=top_ps[i], banned=ban[i], **KW)
            assert one == got[i], i
        # ... and the parameters matter: stream 0 at stream 2's values is another piece
        assert _alone(inf, model, e2i, i2e, leads[0], primers[0], big.U[:, 0], temp=temps[2], top_p=top_ps[2], **KW) != got[0]
    api, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, temp=temps, top_p=top_ps, banned=ban, **KW)
    assert api == got


def test_the_queue_gives_every_job_the_controls_it_has_in_lock_step(s2):
    inf, model, e2i, i2e, leads, primers = s2
    ctl = dict(temp=[0.8, 1.2, 1.7], top_p=[0.9, 0.97, 0.6], banned=[[e2i['Beat_0'], e2i['Beat_1']], None, [e2i['Chord_I_M'], e2i['Note_Degree_1']]])
    lock, _, sl = inf.generate_accompaniments(model, e2i, i2e, leads, primers, return_scores=True, **ctl, **KW)
    queue, _, sq = inf.generate_accompaniments(model, e2i, i2e, leads, primers, slots=2, return_scores=True, **ctl, **KW)
    assert queue == lock
    for i in (0, 2):
        assert not {t for _, t in drawn(queue[i], sq[i])[0]} & set(ctl['banned'][i])
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, slots=2, **KW)
    assert all(a != b for a, b in zip(plain, queue))


def test_best_of_gives_both_candidates_the_inputs_controls(s2):
    inf, model, e2i, i2e, leads, primers = s2
    base, _, _, sc0 = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=2, best_by='draws', return_scores=True, **KW)
    ban = [sorted(favourites(base[:1], sc0[:1], spare={e2i['Track_LeadSheet'], e2i['EOS_None']})), None, [e2i['Beat_2']]]
    got, _, picks, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=2, best_by='draws', return_scores=True, banned=ban,
                                                   temp=[1.0, 1.2, 1.4], **KW)
    for i, p in enumerate(picks):
        assert len(p['candidates']) == 2
        for ids, sc in zip(p['candidates'], p['scores']):
            assert not isinstance(ids, Exception)
            d, _ = drawn(ids, sc)
            assert d and (ban[i] is None or not {t for _, t in d} & set(ban[i])), (i, d)
    loop = inf.AccompanimentLoop(model, e2i, i2e, [x for x in leads for _ in range(2)], [x for x in primers for _ in range(2)], banned=[b for b in ban for _ in range(2)],
                                 temp=[t for t in (1.0, 1.2, 1.4) for _ in range(2)], **KW)
    assert loop.control_tables['mask_of'].tolist() == [0, 0, -1, -1, 1, 1]
    assert loop.control_tables['temp_of'].tolist() == [np.float32(t) for t in (1.0, 1.0, 1.2, 1.2, 1.4, 1.4)]


def _long(s2, monkeypatch):
    inf, model, e2i, i2e, leads, primers = s2
    monkeypatch.setattr(inf, 'max_dec_inp_len', 24)
    g = s2b._vocab()[0]
    lead = [list(b) for b in g['lead']]
    return [lead * 4, [lead[2]], lead * 3], primers, dict(max_events=70, skip_check=False, seed=9)


def test_a_stream_past_the_window_keeps_its_ban_on_the_device(s2, monkeypatch):
    inf, model, e2i, i2e = s2[:4]
    leads, primers, kw = _long(s2, monkeypatch)

    def run(**ctl):
        loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, scores=True, **ctl, **kw)
        loop.run()
        out = loop.results(e2i, i2e, kw['max_events'], False, kw['seed'], window='device')
        return loop, out, loop.scores(out)

    loop, base, sc = run()
    assert loop.windowed is not None and 0 in loop.windowed.idx
    past = Counter(t for c, t in drawn(base[0], sc[0])[0] if c >= 24 and t not in (e2i['Track_LeadSheet'], e2i['EOS_None']))
    ban = sorted(t for t, _ in past.most_common(3))
    assert ban
    loop, got, sc = run(banned=[ban, None, None], temp=[1.3, 1.2, 1.2])
    w = loop.windowed
    assert w is not None and 0 in w.idx
    j = w.idx.index(0)
    assert w.controls.bans[j] == tuple(ban) and w.controls.temp_at(j) == 1.3
    assert w.control_tables['mask_of'].tolist()[j] == 0 and abs(w.control_tables['temp_of'].tolist()[j] - 1.3) < 1e-6
    assert all(w.controls.bans[k] is None for k in range(len(w.idx)) if k != j)
    d = [(c, t) for c, t in drawn(got[0], sc[0])[0] if c >= 24]
    assert len(d) >= 5 and not {t for _, t in d} & set(ban), d


def test_the_hand_over_to_the_host_finish_passes_the_ban_and_the_temperature_on(s2, monkeypatch):
    inf, model, e2i, i2e = s2[:4]
    leads, primers, kw = _long(s2, monkeypatch)
    calls, real = [], inf._resume_windowed

    def spy(model_, e2i_, i2e_, s, max_events, skip_check, temp, inadmissibles, sampler):
        calls.append((list(s.generated[:3]), temp, inadmissibles))
        return real(model_, e2i_, i2e_, s, max_events, skip_check, temp, inadmissibles, sampler)

    monkeypatch.setattr(inf, '_resume_windowed', spy)
    ban = [e2i['Beat_5'], e2i['Beat_3'], e2i['Chord_V_M']]
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, banned=[ban, None, None], temp=[1.3, 1.2, 1.1], window='host', **kw)
    by_primer = {tuple(c[0]): c for c in calls}
    assert tuple(primers[0]) in by_primer
    _, temp, inadm = by_primer[tuple(primers[0])]
    assert temp == 1.3 and sorted(inadm) == sorted(ban)
    for k, c in by_primer.items():
        if k != tuple(primers[0]):
            assert c[2] is None and c[1] == {tuple(primers[1]): 1.2, tuple(primers[2]): 1.1}[k]
    assert not isinstance(got[0], Exception)
    # past the hand-off the host loop draws under the same ban (its `inadmissibles`): no banned id behind the window but a given one
    given = {t for bar in leads[0] for t in bar} | {e2i['Track_Full'], e2i['Track_LeadSheet']}
    assert not (set(got[0][24:]) & set(ban)) - given


def test_key_ban_forces_the_key_in_stage_one():
    from emo_disentanger_amd import stage1_inference as s1
    _, m, e2i, i2e = s1b._fixture('fp32')
    keys = [i for e, i in e2i.items() if e.startswith('Key_')]
    with torch.no_grad():
        m.dec_out_proj.bias[keys] += 30.0                          # a model that answers the emotion tag with a key, any key
    primers = [['Emotion_Q1'], ['Emotion_Positive'], ['Emotion_Q1'], ['Emotion_Positive']]
    kw = dict(representation='functional', key_determine='rule', max_bars=2, max_events=12, seed=4)
    forced, _, sc = s1.generate_lead_sheets(m, e2i, i2e, primers, banned=s1.key_ban(e2i, 'Key_G'), return_scores=True, **kw)
    assert all(isinstance(r, list) and r[1] == e2i['Key_G'] for r in forced), forced          # never KEY_ERROR, never another key
    assert all(s['rank'][1] >= 0 for s in sc)                      # ... and it was drawn, not given
    other = set(keys) - {e2i['Key_G']}
    assert not any(set(r[1:]) & other for r in forced)
    # per primer: only the second is forced, through a queue of two slots
    mixed, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, banned=[None, s1.key_ban(e2i, 'Key_C'), None, None], slots=2, temp=[1.2, 1.0, 1.2, 1.2], **kw)
    assert isinstance(mixed[1], list) and mixed[1][1] == e2i['Key_C']
