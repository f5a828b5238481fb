"""CPU: the host side of classifier-free valence guidance in the stage-1 device draw (emo_grammar_step, kind TXL: guide_cond / guide_uncond /
guide_scale): the entry's new refusal behind every existing one of the kind (nothing is launched), every refusal of
generate_lead_sheets(guidance=, uncond=) before a loop is built, the follower primers and the emotion mode they inherit, the loop classes that
take the tables, the renumbering of the pairs under best_of, the pair check on stage-1 results, and the command line."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

NEW = ['guide_cond', 'guide_uncond', 'guide_scale']
TXL, TXL_QUEUE = 0, 3


# ------------------------------------------------------------------------------------------------ the entry
def _args(kind, **kw):
    """A block that passes every host check of `kind` (pointer fields: small fake addresses - validation never dereferences them, and no refusal
    below gets as far as the launch), with the fields of `kw` changed."""
    from emo_disentanger_amd import _lib
    a = _lib.GrammarStep()
    for name, ctype in _lib.GrammarStep._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.kind, a.n_rows, a.n_token, a.n_u, a.ld_u, a.ld_seq, a.max_len, a.window = kind, 3, 200, 8, 3, 64, 32, 32
    a.n_jobs, a.mem_rows = 3, 32
    a.temperature, a.top_p, a.key_temperature, a.key_top_p = 1.2, 0.9, 1.1, 0.97
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refusal(a):
    from emo_disentanger_amd import _lib
    assert _lib.lib.emo_grammar_step(ctypes.byref(a), None) == -1
    return _lib.lib.emo_last_error().decode()


PART = NEW + [('guide_cond', 'guide_uncond'), ('guide_uncond', 'guide_scale'), ('guide_cond', 'guide_scale')]


@pytest.mark.parametrize('missing', PART)
def test_kind_txl_refuses_one_or_two_of_the_three(missing):
    missing = (missing,) if isinstance(missing, str) else missing
    msg = _refusal(_args(TXL, **{k: None for k in missing}))
    assert msg == 'emo_grammar_step[txl]: guide_cond, guide_uncond and guide_scale come together or not at all'


FIRST = [(dict(n_token=2000), 'V must be <= 1024 (got 2000)'), (dict(temperature=0.0), 'temperatures must be > 0'),
         (dict(key_temperature=0.0), 'temperatures must be > 0'), (dict(tok_out=None), 'null pointer'), (dict(logits=None), 'null pointer'),
         (dict(n_u=0), 'bad sizes'), (dict(ld_u=2), 'bad sizes')]


@pytest.mark.parametrize('kw, what', FIRST)
@pytest.mark.parametrize('guide', ['all', 'none'] + PART, ids=lambda g: g if isinstance(g, str) else '+'.join(g))
def test_kind_txl_keeps_its_first_refusals_whatever_the_three_fields_hold(kw, what, guide):
    # all three fake pointers, none, or any one or two of them: the new check comes behind every other one of the kind
    missing = () if guide == 'all' else NEW if guide == 'none' else (guide,) if guide in NEW else guide
    assert _refusal(_args(TXL, **kw, **{k: None for k in missing})) == 'emo_grammar_step[txl]: %s' % what


@pytest.mark.parametrize('missing', PART)
def test_kind_txl_queue_does_not_look_at_the_three_fields(missing):
    missing = (missing,) if isinstance(missing, str) else missing
    for kw, what in ((dict(key_temperature=0.0), 'temperatures must be > 0'), (dict(n_jobs=0), 'bad sizes'), (dict(slot_job=None), 'null pointer')):
        assert _refusal(_args(TXL_QUEUE, **kw, **{k: None for k in missing})) == 'emo_grammar_step[txl_queue]: %s' % what


# ------------------------------------------------------------------------------------------------ generate_lead_sheets
VOCAB = ['Emotion_Positive', 'Emotion_Negative', 'Emotion_None', 'Key_C', 'Key_a', 'Bar_None', 'Beat_0', 'Beat_4', 'Note_Degree_1', 'EOS_None', 'PAD_None']
E2I = {e: i for i, e in enumerate(VOCAB)}
I2E = dict(enumerate(VOCAB))
PRIMERS = [['Emotion_Positive'], ['Key_C', 'Emotion_Negative', 'Bar_None'], ['Emotion_Negative', 'Key_a']]


def _fake_model(V=40):
    m = SimpleNamespace(training=False, n_token=V, vocab_size=V, calls=[], _max_gen_len=64)
    m.eval = lambda: m.calls.append('eval')
    m.train = lambda mode=True: m.calls.append(('train', mode))
    m.parameters = lambda: iter([torch.zeros(1)])
    return m


BAD_CALLS = [
    (dict(guidance=1.5, slots=2), E2I, PRIMERS, 'slots'),
    (dict(guidance=[0.0, None, 2.0], slots=4), E2I, PRIMERS, 'slots'),
    (dict(guidance=-0.5), E2I, PRIMERS, 'finite scale >= 0'), (dict(guidance=[1.0, float('inf'), 0.0]), E2I, PRIMERS, 'finite scale >= 0'),
    (dict(guidance=float('nan')), E2I, PRIMERS, 'finite scale >= 0'), (dict(guidance='x'), E2I, PRIMERS, 'guidance'),
    (dict(guidance=[1.0, 2.0]), E2I, PRIMERS, 'guidance has 2 entries for 3 inputs'),
    (dict(guidance=[1.0, 2.0, 1.0, 1.0]), E2I, PRIMERS, 'guidance has 4 entries for 3 inputs'),
    (dict(guidance=1.5), {k: v for k, v in E2I.items() if k != 'Emotion_None'}, PRIMERS, 'no Emotion_None'),
    (dict(guidance=1.5), E2I, [['Emotion_Positive'], ['Key_C', 'Bar_None'], ['Emotion_Negative']], 'primer 1 has no Emotion_'),
    (dict(guidance=1.5), E2I, [['Emotion_Positive'], None, ['Emotion_Negative']], 'primer 1 has no Emotion_'),
    (dict(guidance=1.5, uncond=40), E2I, PRIMERS, r'token id in \[0, 40\)'), (dict(guidance=1.5, uncond=-1), E2I, PRIMERS, r'token id in \[0, 40\)'),
    (dict(guidance=1.5, uncond=2.0), E2I, PRIMERS, 'event name or a token id'), (dict(guidance=1.5, uncond='Emotion_Q9'), E2I, PRIMERS, 'not an event'),
    (dict(guidance=1.5), dict(E2I, Emotion_None=40), PRIMERS, r'outside \[0, 40\)'),
]


@pytest.mark.parametrize('kw, e2i, primers, what', BAD_CALLS)
def test_generate_lead_sheets_refuses_before_anything_is_allocated(monkeypatch, kw, e2i, primers, what):
    from emo_disentanger_amd import stage1_inference as s1

    def never(*a, **k):
        raise AssertionError('a loop was built')

    for name in ('LeadSheetLoop', 'LeadSheetQueue'):
        monkeypatch.setattr(s1, name, never)
    for extra in ({}, {'best_of': 2}, {'step': 'one_launch'}):
        with pytest.raises(ValueError, match=what):
            s1.generate_lead_sheets(_fake_model(), e2i, I2E, primers, **kw, **extra)


class _FakeLoop:
    built = []

    def __init__(self, model, e2i, i2e, primers, **kw):
        self.built.append((primers, kw))
        self.n = len(primers)
        self.state = torch.zeros(self.n, 8, dtype=torch.int32)
        self.state[:, 0] = 1                                                       # DONE
        self.params = torch.zeros(self.n, 8, dtype=torch.int32)
        self.params[:, 2] = torch.tensor([len(p) for p in primers])

    def run(self, use_graph=True):
        pass

    def results(self):
        return [[t if isinstance(t, int) else E2I[t] for t in p] + [5, 8] for p in self.built[-1][0]]

    def scores(self):
        return [{'logp': np.full(len(r), -1.0 - i, np.float32), 'rank': np.zeros(len(r), np.int32), 'entropy': np.ones(len(r), np.float32)}
                for i, r in enumerate(self.results())]


def test_a_guided_call_builds_one_lock_step_loop_with_the_followers_behind_the_leaders(monkeypatch):
    from emo_disentanger_amd import scoring, stage1_inference as s1
    built = _FakeLoop.built = []
    monkeypatch.setattr(s1, 'LeadSheetLoop', _FakeLoop)
    monkeypatch.setattr(s1, 'LeadSheetQueue', lambda *a, **k: (_ for _ in ()).throw(AssertionError('a queue was built')))
    scored = []
    monkeypatch.setattr(scoring, 'lead_sheet_candidate_scores',
                        lambda model, cands, plens: scored.append((list(cands), list(plens))) or [float(i) for i in range(len(cands))])
    ids = [[E2I[e] for e in p] for p in PRIMERS]
    out, _, sc = s1.generate_lead_sheets(_fake_model(), E2I, I2E, PRIMERS, guidance=[1.5, None, 0.5], temp=[1.0, 1.1, 1.2], banned=[[9], None, None],
                                         max_bars=[4, 5, 6], key_determine=['rule', None, 'rule'], max_events=100, return_scores=True)
    primers, kw = built[-1]
    # the follower is its leader's primer with the FIRST Emotion_ token replaced by Emotion_None; its other options are its leader's
    assert primers == PRIMERS + [[2], [2, 4]]
    assert kw['guidance'] == ([0, -1, 2, 0, 2], [3, -1, 4, 3, 4], [1.5, 0.0, 0.5, 1.5, 0.5])
    assert kw['max_bars'] == [4, 5, 6, 4, 6] and kw['key_determine'] == ['rule', None, 'rule', 'rule', 'rule'] and kw['max_events'] == 100
    assert kw['temp'] == [1.0, 1.1, 1.2, 1.0, 1.2] and kw['banned'] == [(9,), None, None, (9,), None]
    assert out == [p + [5, 8] for p in ids]                                        # the followers are gone
    assert len(sc) == 3 and 'logp_uncond' not in sc[1]
    assert sc[0]['logp_uncond'].tolist() == [-4.0] * 3 and sc[2]['logp_uncond'].tolist() == [-5.0] * 4 and sc[0]['logp'].tolist() == [-1.0] * 3
    # uncond as an event name or an id: contrastive prompting; the emotion token wherever it stands
    for unc in ('Emotion_Positive', 0):
        s1.generate_lead_sheets(_fake_model(), E2I, I2E, PRIMERS, guidance=[None, 2.0, 0], uncond=unc)
        assert built[-1][0] == PRIMERS + [[3, 0, 5]] and built[-1][1]['guidance'] == ([-1, 1, -1, 1], [-1, 3, -1, 3], [0.0, 2.0, 0.0, 2.0])
    # best_of: candidate c of a leader is paired with candidate c of its follower; leaders keep rows [0, n * N); the leaders alone are scored
    chosen, _, picks = s1.generate_lead_sheets(_fake_model(), E2I, I2E, PRIMERS, guidance=[1.5, None, 0.5], best_of=2, max_bars=[4, 5, 6])
    primers, kw = built[-1]
    assert primers == [p for p in PRIMERS + [[2], [2, 4]] for _ in range(2)] and kw['max_bars'] == [4, 4, 5, 5, 6, 6, 4, 4, 6, 6]
    assert kw['guidance'][0] == [0, 1, -1, -1, 4, 5, 0, 1, 4, 5] and kw['guidance'][1] == [6, 7, -1, -1, 8, 9, 6, 7, 8, 9]
    assert kw['guidance'][2] == [1.5, 1.5, 0.0, 0.0, 0.5, 0.5, 1.5, 1.5, 0.5, 0.5]
    assert len(picks) == 3 and all(len(p['candidates']) == 2 for p in picks) and chosen == [p + [5, 8] for p in ids]
    assert [p['nll_mean'] for p in picks] == [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]]
    assert len(scored[-1][0]) == 6 and scored[-1][1] == [1, 1, 3, 3, 2, 2]           # six leaders and their primer lengths, no follower
    _, _, picks, sc = s1.generate_lead_sheets(_fake_model(), E2I, I2E, PRIMERS, guidance=1.5, best_of=2, best_by='draws', return_scores=True)
    assert all('logp_uncond' in s for p in picks for s in p['scores']) and all('logp_uncond' in s for s in sc)
    assert [p['nll_mean'] for p in picks] == [[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]]  # ranked by the leaders' own tables
    # guidance off: the loop is built as it is without the argument
    for g in (None, 0.0, [0, None, 0]):
        s1.generate_lead_sheets(_fake_model(), E2I, I2E, PRIMERS, guidance=g)
        assert built[-1][0] == PRIMERS and 'guidance' not in built[-1][1]
    s1.generate_lead_sheets(_fake_model(), E2I, I2E, PRIMERS, guidance=None, uncond='nonsense')      # (uncond without guidance is not looked at)


def _loaded(primers, guidance, **per_stream):
    """LeadSheetLoop._load_jobs on host tensors: the job tables of a loop without its model memory."""
    from emo_disentanger_amd import stage1_inference as s1
    loop = s1.LeadSheetLoop.__new__(s1.LeadSheetLoop)
    kw = dict(max_bars=8, max_events=50, prompt_bars=None, representation='functional', key_determine='rule')
    kw.update(per_stream)
    plens = loop._load_jobs(_fake_model(), E2I, I2E, primers, 1.2, 0.9, None, None, guidance, **kw)
    return loop, plens


def test_a_follower_inherits_its_leaders_emotion_mode_and_options():
    from emo_disentanger_amd import stage1_inference as s1
    primers = [['Emotion_Positive'], ['Emotion_None'], ['Emotion_Negative'], [2], [E2I['Emotion_Positive']]]
    guide = ([0, -1, 2, 0, 2], [3, -1, 4, 3, 4], [1.5, 0.0, 0.5, 1.5, 0.5])
    loop, plens = _loaded(primers, guide, max_bars=[4, 5, 6, 4, 6])
    p = loop.params.numpy()
    assert plens == [1] * 5 and loop.seq[:, 0].tolist() == [0, 2, 1, 2, 0]
    # Emotion_None alone has mode 0 (stream 1); follower 3 (Emotion_None) has Positive's 1, follower 4 (contrastive: Positive) Negative's 2
    assert p[:, s1.P_EMO_MODE].tolist() == [1, 0, 2, 1, 2]
    assert np.array_equal(p[3], p[0]) and np.array_equal(p[4], p[2]) and p[:, s1.P_KEY_RULE].tolist() == [1] * 5
    assert loop.job_controls.followers() == [3, 4] and int(loop.running.item()) == 5
    # without guidance every stream has its own tag's mode
    loop, _ = _loaded(primers, None)
    assert loop.params.numpy()[:, s1.P_EMO_MODE].tolist() == [1, 0, 2, 0, 1] and loop.job_controls.guide_arg is None
    # a follower in front of a leader, or one that differs from its leader in an option or in its primer's length
    with pytest.raises(ValueError, match='behind every other stream'):
        _loaded(primers[:2], ([1, 1], [0, 0], [1.0, 1.0]))
    with pytest.raises(ValueError, match='differ in primer length or in a per-stream option'):
        _loaded(primers, guide, max_bars=[4, 5, 6, 7, 6])
    with pytest.raises(ValueError, match='differ in primer length or in a per-stream option'):
        _loaded(primers[:3] + [[2, 3]] + primers[4:], guide)


def test_the_lock_step_stage1_loop_takes_the_tables_and_the_queue_does_not(monkeypatch):
    from emo_disentanger_amd import gen_loop as gl, ops, stage1_inference as s1
    from emo_disentanger_amd._lib import EmoError
    monkeypatch.setattr(ops, 'ptr', lambda t: None if t is None else t.data_ptr())
    ctl = gl.draw_controls('t', 3, 40, None, 1.2, 0.9).with_guidance([1.5, 0.0, 0.5])
    num = dict(n_rows=5, n_token=40, ld_u=5, temperature=1.2, top_p=0.9)

    def fresh(cls):
        loop = cls.__new__(cls)
        loop.dev, loop.seq = 'cpu', torch.zeros(5, 16, dtype=torch.int64)
        return loop

    loop = fresh(s1.LeadSheetLoop)
    loop._build_block(ops.GRAMMAR_TXL, False, ctl, **num)
    a, t = loop._gargs, loop.control_tables
    assert sorted(t) == sorted(NEW) and all(getattr(a, k) == t[k].data_ptr() and loop._gheld[k] is t[k] for k in NEW)
    assert t['guide_cond'].tolist() == [0, -1, 2, 0, 2] and t['guide_uncond'].tolist() == [3, -1, 4, 3, 4] and t['guide_scale'].tolist() == [1.5, 0.0, 0.5, 1.5, 0.5]
    for cls, kind in ((s1.LeadSheetLoop, ops.GRAMMAR_TXL_QUEUE), (s1.LeadSheetQueue, ops.GRAMMAR_TXL_QUEUE), (s1.LeadSheetLoop, ops.GRAMMAR_ACC),
                      (gl.GrammarLoop, ops.GRAMMAR_TXL)):
        with pytest.raises(EmoError, match='guidance pairs'):
            fresh(cls)._build_block(kind, False, ctl, **num)
    loop = fresh(s1.LeadSheetLoop)
    loop._build_block(ops.GRAMMAR_TXL, False, gl.draw_controls('t', 5, 40, None, 1.2, 0.9), **num)
    assert all(getattr(loop._gargs, k) is None for k in NEW) and loop.control_tables == {}


def test_the_pair_check_reads_stage1_results():
    from emo_disentanger_amd import gen_loop as gl, inference as inf
    from emo_disentanger_amd._lib import EmoError
    ctl = gl.draw_controls('t', 3, 40, None, 1.2, 0.9).with_guidance([1.0, 1.0, 1.0])
    err = ValueError('[info] key generation failed')
    res = [[0, 3, 7], None, err, [2, 3, 7], None, ValueError('[info] key generation failed')]
    out, _ = inf.check_pairs(res, [1, 2, 3, 1, 2, 3], None, ctl, [0, 0, 0], who='generate_lead_sheets')
    assert out == [[0, 3, 7], None, err]                                           # a pair that got stuck, or failed on the key, together stays what it is
    out, _ = inf.check_pairs([[0, 3, 7], None, err, [2, 4, 7], [2, 5], None], [1, 2, 3, 1, 1, 2], None, ctl, [0, 0, 0], who='generate_lead_sheets')
    assert all(isinstance(o, EmoError) and str(o).startswith('generate_lead_sheets: stream') for o in out)
    assert 'token 1' in str(out[0]) and 'status 2 against 1' in str(out[1]) and 'status 3 against 2' in str(out[2])


# ------------------------------------------------------------------------------------------------ command line
def test_the_guidance_flags_and_their_refusals():
    from emo_disentanger_amd import stage1_inference as s1
    base = ['-c', 'conf.yaml', '-r', 'functional', '-m', 'lead_sheet']
    a = s1.parse_args(base)
    assert a.guidance is None and a.uncond is None
    assert s1.parse_args(base + ['--guidance', '1.5']).guidance == 1.5
    a = s1.parse_args(base + ['--guidance', '2', '--uncond', 'Emotion_Negative', '--best-of', '2', '--step', 'one-launch'])
    assert a.guidance == 2.0 and a.uncond == 'Emotion_Negative'
    assert s1.parse_args(base + ['--guidance', '0', '--slots', '4']).guidance == 0.0      # no piece is guided: the queue may run
    for bad in (['--guidance', '1.5', '--slots', '4'], ['--guidance', '-1'], ['--guidance', 'inf'], ['--guidance', 'nan'], ['--guidance', '1.5', '--exact'],
                ['--uncond', 'Emotion_None']):
        with pytest.raises(SystemExit):
            s1.parse_args(base + bad)
