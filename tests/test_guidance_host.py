"""CPU: the host side of classifier-free emotion guidance in the stage-2 device draw (emo_grammar_step_t: guide_cond / guide_uncond / guide_scale):
the ctypes mirror, the entry's refusals with the fields set (nothing is launched), block_set's checks of the three tables, every refusal of
generate_accompaniments(guidance=, uncond=) before a loop is built, the follower primers, DrawControls' renumbering of the pairs under repeat /
take, the pair check of the results, and the command line."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

NEW = ['guide_cond', 'guide_uncond', 'guide_scale']
KIND_NAME = {0: 'txl', 1: 'acc', 2: 'acc_window', 3: 'txl_queue', 4: 'acc_queue'}


# ------------------------------------------------------------------------------------------------ the block
def test_the_mirror_holds_the_three_fields_among_the_acc_fields_in_front_of_job_steps():
    from emo_disentanger_amd import _lib
    G = _lib.GrammarStep
    names = [f[0] for f in G._fields_]
    at = names.index('guide_cond')
    assert names[at:at + 3] == NEW and at + 3 <= names.index('job_steps')
    assert names[at - 1] == 'pad' and names[at + 3] == 'segs'              # among the fields kind ACC reads, in front of ACC_WINDOW's run
    assert all(dict(G._fields_)[k] is _lib.c_p for k in NEW)
    assert _lib.lib.emo_grammar_step_size() == ctypes.sizeof(G)
    off = G.pad.offset
    for k in NEW:
        off += 8
        assert getattr(G, k).offset == off and getattr(G, k).size == 8, k
    a = G()
    assert a.guide_cond is None and a.guide_uncond is None and a.guide_scale is None


def _args(kind, **kw):
    """A block that passes every host check of `kind` (pointer fields: small fake addresses - validation never dereferences them, and no refusal
    below gets as far as the launch), with the fields of `kw` changed."""
    from emo_disentanger_amd import _lib
    a = _lib.GrammarStep()
    for name, ctype in _lib.GrammarStep._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.kind, a.n_rows, a.n_token, a.n_u, a.ld_u, a.ld_seq, a.max_len, a.window = kind, 3, 327, 8, 3, 64, 32, 32
    a.n_jobs, a.mem_rows = 3, 32
    a.temperature, a.top_p, a.key_temperature, a.key_top_p = 1.2, 0.9, 1.1, 0.97
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refusal(a):
    from emo_disentanger_amd import _lib
    assert _lib.lib.emo_grammar_step(ctypes.byref(a), None) == -1
    return _lib.lib.emo_last_error().decode()


@pytest.mark.parametrize('missing', NEW + [('guide_cond', 'guide_uncond'), ('guide_uncond', 'guide_scale'), ('guide_cond', 'guide_scale')])
def test_kind_acc_refuses_one_or_two_of_the_three(missing):
    missing = (missing,) if isinstance(missing, str) else missing
    msg = _refusal(_args(1, **{k: None for k in missing}))
    assert msg == 'emo_grammar_step[acc]: guide_cond, guide_uncond and guide_scale come together or not at all'


# what every kind answers to one defect, as the entry answered before the fields existed (tests/test_abi.py, tests/test_stage2_queue_host.py)
FIRST = [
    (0, dict(n_token=2000), 'V must be <= 1024 (got 2000)'), (1, dict(n_token=2000), 'V must be <= 1024 (got 2000)'),
    (2, dict(n_token=2000), 'V must be <= 1024 (got 2000)'), (3, dict(n_token=2000), 'V must be <= 1024 (got 2000)'),
    (4, dict(n_token=2000), 'V must be <= 1024 (got 2000)'),
    (0, dict(temperature=0.0), 'temperatures must be > 0'), (1, dict(temperature=0.0), 'temperature must be > 0'),
    (2, dict(temperature=0.0), 'temperature must be > 0'), (3, dict(key_temperature=0.0), 'temperatures must be > 0'),
    (4, dict(temperature=0.0), 'temperature must be > 0'),
    (0, dict(tok_out=None), 'null pointer'), (1, dict(seg_out=None), 'null pointer'), (2, dict(win_seg=None), 'null pointer'),
    (3, dict(slot_job=None), 'null pointer'), (4, dict(row_reset=None), 'null pointer'),
    (0, dict(n_u=0), 'bad sizes'), (1, dict(max_len=0), 'bad sizes'), (2, dict(window=65), 'bad sizes'), (3, dict(n_jobs=0), 'bad sizes'),
    (4, dict(mem_rows=0), 'bad sizes'),
]


@pytest.mark.parametrize('kind, kw, what', FIRST)
@pytest.mark.parametrize('guide', ['all', 'none', 'two'])
def test_every_kind_keeps_its_first_refusal_whatever_the_three_fields_hold(kind, kw, what, guide):
    # all three fake pointers, none, or two of them: the new check comes behind every other one, and no kind but ACC makes it at all
    more = {} if guide == 'all' else {k: None for k in (NEW if guide == 'none' else NEW[1:2])}
    assert _refusal(_args(kind, **kw, **more)) == 'emo_grammar_step[%s]: %s' % (KIND_NAME[kind], what)


# ------------------------------------------------------------------------------------------------ block_set
def _tables(c, g, s):
    return dict(guide_cond=torch.tensor(c, dtype=torch.int32), guide_uncond=torch.tensor(g, dtype=torch.int32),
                guide_scale=torch.tensor(s, dtype=torch.float32))


GOOD = ([0, -1, 2, 0, 2], [3, -1, 4, 3, 4], [1.5, 0.0, 0.0, 1.5, 0.0])       # rows 0 / 3 and 2 / 4 are pairs, row 1 is unguided
BAD_TABLES = [
    (([0, -1, 2, 0, 2], [3, -1, 5, 3, 4], GOOD[2]), 'outside'),               # an index out of range
    (([0, -1, 2, 0, 2], [3, -1, -2, 3, 4], GOOD[2]), 'outside'),
    (([0, 1, 2, 0, 2], [3, -1, 4, 3, 4], GOOD[2]), 'outside'),                # half a pair
    (([0, 1, 2, 0, 2], [3, 1, 4, 3, 4], GOOD[2]), 'names one row twice'),     # a self-pair
    (([0, 0, 2, 0, 2], [3, 3, 4, 3, 4], GOOD[2]), 'neither row'),             # a third row on a pair
    (([0, -1, 2, 0, 2], [3, -1, 4, 3, 3], GOOD[2]), 'disagree'),              # a follower whose pair differs from its leader's ...
    (([0, -1, 2, 0, 4], [3, -1, 4, 3, 2], GOOD[2]), 'disagree'),              # ... the two rows swapped on one side
    ((GOOD[0], GOOD[1], [1.5, 0.0, 0.0, 2.5, 0.0]), 'disagree'),              # ... another scale
    ((GOOD[0], GOOD[1], [-1.0, 0.0, 0.0, -1.0, 0.0]), 'not a finite scale'),
    ((GOOD[0], GOOD[1], [1.5, 0.0, float('inf'), 1.5, float('inf')]), 'not a finite scale'),
    ((GOOD[0], GOOD[1], [1.5, float('nan'), 0.0, 1.5, 0.0]), 'not a finite scale'),
]


def test_block_set_takes_a_sound_set_and_refuses_every_other(monkeypatch):
    from emo_disentanger_amd import ops
    monkeypatch.setattr(ops, 'ptr', lambda t: None if t is None else t.data_ptr())
    args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
    ops.block_set(args, held, n_rows=5, ld_u=5, n_token=40, **_tables(*GOOD))
    assert all(getattr(args, k) == held[k].data_ptr() for k in NEW)
    for tabs, what in BAD_TABLES:
        args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
        with pytest.raises(AssertionError, match=what):
            ops.block_set(args, held, n_rows=5, ld_u=5, n_token=40, **_tables(*tabs))
        assert all(getattr(args, k) is None for k in NEW) and not any(k in held for k in NEW)       # a refused set never stays in the block
        assert ops.guide_pairs_error(*tabs) is not None and what in ops.guide_pairs_error(*tabs)
    assert ops.guide_pairs_error(*GOOD) is None
    # one or two of the three; the wrong length or type
    for keys in (NEW[:1], NEW[:2], NEW[1:]):
        with pytest.raises(AssertionError, match='come together'):
            ops.block_set(ops.GrammarStep(), {}, n_rows=5, ld_u=5, n_token=40, **{k: _tables(*GOOD)[k] for k in keys})
    with pytest.raises(AssertionError, match='guide_cond'):
        ops.block_set(ops.GrammarStep(), {}, n_rows=4, ld_u=4, n_token=40, **_tables(*GOOD))
    with pytest.raises(AssertionError, match='guide_scale'):
        ops.block_set(ops.GrammarStep(), {}, n_rows=5, ld_u=5, n_token=40, **dict(_tables(*GOOD), guide_scale=torch.zeros(5, dtype=torch.float64)))


# ------------------------------------------------------------------------------------------------ generate_accompaniments
VOCAB = ['Emotion_Q1', 'Emotion_Q2', 'Emotion_None', 'Key_C', 'Tempo_110', 'Track_LeadSheet', 'Track_Full', 'Bar_None', 'Beat_0', 'PAD_None']
E2I = {e: i for i, e in enumerate(VOCAB)}
I2E = dict(enumerate(VOCAB))
LEADS = [[[7, 8]], [[7]], [[7, 8]]]
PRIMERS = [[0, 3, 4], [3, 1, 4], [0, 4]]


def _fake_model(V=40):
    m = SimpleNamespace(training=False, n_token=V, vocab_size=V, calls=[])
    m.eval = lambda: m.calls.append('eval')
    m.train = lambda mode=True: m.calls.append(('train', mode))
    return m


BAD_CALLS = [
    (dict(guidance=1.5, slots=2), E2I, PRIMERS, 'slots'),
    (dict(guidance=[0.0, None, 2.0], slots=4), E2I, PRIMERS, 'slots'),
    (dict(guidance=1.5, window='device'), E2I, PRIMERS, "window='device'"),
    (dict(guidance=1.5), {k: v for k, v in E2I.items() if k != 'Emotion_None'}, PRIMERS, 'no Emotion_None'),
    (dict(guidance=1.5), E2I, [[0, 3, 4], [3, 4], [0, 4]], 'primer 1 has no Emotion_'),
    (dict(guidance=1.5, uncond=2), {}, [[0, 3, 4], [3, 4], [0, 4]], 'primer 1 has no Emotion_'),
    (dict(guidance=[1.0, 2.0]), E2I, PRIMERS, 'guidance has 2 entries for 3 inputs'),
    (dict(guidance=[1.0, 2.0, 1.0, 1.0]), E2I, PRIMERS, 'guidance has 4 entries for 3 inputs'),
    (dict(guidance=-0.5), E2I, PRIMERS, 'finite scale >= 0'), (dict(guidance=[1.0, float('inf'), 0.0]), E2I, PRIMERS, 'finite scale >= 0'),
    (dict(guidance=float('nan')), E2I, PRIMERS, 'finite scale >= 0'), (dict(guidance='x'), E2I, PRIMERS, 'guidance'),
]


@pytest.mark.parametrize('kw, e2i, primers, what', BAD_CALLS)
def test_generate_accompaniments_refuses_before_anything_is_allocated(monkeypatch, kw, e2i, primers, what):
    from emo_disentanger_amd import inference as inf

    def never(*a, **k):
        raise AssertionError('a loop was built')

    for name in ('AccompanimentLoop', 'AccompanimentQueue'):
        monkeypatch.setattr(inf, name, never)
    for extra in ({}, {'best_of': 2}):
        with pytest.raises(ValueError, match=what):
            inf.generate_accompaniments(_fake_model(), e2i, I2E, LEADS, primers, **kw, **extra)


def test_the_plan_finds_the_emotion_token_and_builds_the_followers():
    from emo_disentanger_amd import inference as inf
    plan = inf.guidance_plan('t', [1.5, None, 0.5], None, E2I, I2E, PRIMERS)
    assert plan.scales == [1.5, 0.0, 0.5] and plan.guided == [0, 2] and plan.emo_pos == [0, None, 0]
    assert plan.followers == [[2, 3, 4], [2, 4]]                                  # the same length, Emotion_None in the emotion's place
    leads, primers = plan.rows(LEADS, PRIMERS)
    assert leads == LEADS + [LEADS[0], LEADS[2]] and primers == PRIMERS + plan.followers
    # the first Emotion_ token wherever it stands; an id given as `uncond` needs no Emotion_None in the vocabulary
    plan = inf.guidance_plan('t', 2.0, 9, {}, I2E, [[3, 1, 4, 0]])
    assert plan.emo_pos == [1] and plan.followers == [[3, 9, 4, 0]]
    # nothing guided: no plan (the call is today's, draw for draw), and no look at the vocabulary
    for g in (None, 0, 0.0, [None, 0, 0.0]):
        assert inf.guidance_plan('t', g, None, {}, {}, PRIMERS) is None


def test_a_guided_call_builds_one_lock_step_loop_with_the_followers_behind_the_leaders(monkeypatch):
    from emo_disentanger_amd import inference as inf, scoring
    built = []

    class Fake:
        bound = 48

        def __init__(self, model, e2i, i2e, leads, primers, **kw):
            built.append((leads, primers, kw))
            self.n = len(leads)
            self.statuses = [1] * self.n

        def run(self, use_graph=True):
            pass

        def results(self, *a, **kw):
            return [[int(t) for t in p] + [5, 8] for p in built[-1][1]]

        def scores(self, results):
            return [{'logp': np.full(len(r), -1.0 - i, np.float32), 'rank': np.zeros(len(r), np.int32), 'entropy': np.ones(len(r), np.float32)}
                    for i, r in enumerate(results)]

    monkeypatch.setattr(inf, 'AccompanimentLoop', Fake)
    monkeypatch.setattr(scoring, 'candidate_scores', lambda model, e2i, cands, max_len: [float(i) for i in range(len(cands))])
    out, _, sc = inf.generate_accompaniments(_fake_model(), E2I, I2E, LEADS, PRIMERS, guidance=[1.5, None, 0.5], temp=[1.0, 1.1, 1.2],
                                             banned=[[9], None, None], return_scores=True)
    leads, primers, kw = built[-1]
    assert primers == PRIMERS + [[2, 3, 4], [2, 4]] and leads == LEADS + [LEADS[0], LEADS[2]]
    assert kw['guidance'] == ([0, -1, 2, 0, 2], [3, -1, 4, 3, 4], [1.5, 0.0, 0.5, 1.5, 0.5])
    assert kw['temp'] == [1.0, 1.1, 1.2, 1.0, 1.2] and kw['banned'] == [(9,), None, None, (9,), None]       # a follower has its leader's controls
    assert out == [p + [5, 8] for p in PRIMERS]                                   # the followers are gone
    assert len(sc) == 3 and 'logp_uncond' not in sc[1]
    assert sc[0]['logp_uncond'].tolist() == [-4.0] * 5 and sc[2]['logp_uncond'].tolist() == [-5.0] * 4 and sc[0]['logp'].tolist() == [-1.0] * 5
    # best_of: candidate c of a leader is paired with candidate c of its follower; leaders keep rows [0, n * N)
    chosen, _, picks = inf.generate_accompaniments(_fake_model(), E2I, I2E, LEADS, PRIMERS, guidance=[1.5, None, 0.5], best_of=2)
    leads, primers, kw = built[-1]
    assert primers == [p for p in PRIMERS + [[2, 3, 4], [2, 4]] for _ in range(2)]
    assert kw['guidance'][0] == [0, 1, -1, -1, 4, 5, 0, 1, 4, 5] and kw['guidance'][1] == [6, 7, -1, -1, 8, 9, 6, 7, 8, 9]
    assert len(picks) == 3 and all(len(p['candidates']) == 2 for p in picks) and chosen == [p + [5, 8] for p in PRIMERS]
    assert [p['nll_mean'] for p in picks] == [[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]]                          # six leaders were scored, no follower
    # guidance off: the loop is built as it is without the argument
    for g in (None, 0.0, [0, None, 0]):
        inf.generate_accompaniments(_fake_model(), E2I, I2E, LEADS, PRIMERS, guidance=g)
        assert built[-1][1] == PRIMERS and 'guidance' not in built[-1][2]


def test_the_pair_check_keeps_sound_pairs_and_marks_the_others():
    from emo_disentanger_amd import gen_loop as gl, inference as inf
    from emo_disentanger_amd._lib import EmoError
    ctl = gl.draw_controls('t', 4, 40, None, 1.2, 0.9).with_guidance([1.0, 0.0, 2.0, 1.0])
    assert ctl.n == 7 and ctl.followers() == [4, 5, 6] and ctl.guide_arg == ([0, -1, 2, 3, 0, 2, 3], [4, -1, 5, 6, 4, 5, 6], [1.0, 0.0, 2.0, 1.0, 1.0, 2.0, 1.0])
    res = [[0, 3, 7], [1, 7], [0, 8, 9], [0, 5], [2, 3, 7], [2, 8, 8], [2, 5, 5]]
    sc = [{'logp': np.arange(len(r), dtype=np.float32) + 10 * i} for i, r in enumerate(res)]
    out, s2 = inf.check_pairs(res, [1] * 7, sc, ctl, [0, None, 0, 0])
    assert out[0] == [0, 3, 7] and out[1] == [1, 7] and len(out) == 4
    assert isinstance(out[2], EmoError) and 'token 2' in str(out[2]) and isinstance(out[3], EmoError) and '2 against 3 tokens' in str(out[3])
    assert s2[0]['logp_uncond'].tolist() == [40.0, 41.0, 42.0] and 'logp_uncond' not in s2[1] and s2[2] is None and s2[3] is None
    assert 'logp_uncond' not in sc[0]                                              # the loop's own dicts are left alone
    # another status word, or one row that failed alone
    out, _ = inf.check_pairs([res[0], res[1], res[4]], [1, 1, 2], None, ctl.take([0, 1, 4]), [0, None])
    assert isinstance(out[0], EmoError) and 'status 1 against 2' in str(out[0]) and out[1] == [1, 7]
    out, _ = inf.check_pairs([res[0], res[1], EmoError('x')], [1, 1, 1], None, ctl.take([0, 1, 4]), [0, None])
    assert isinstance(out[0], EmoError) and 'failed alone' in str(out[0])
    both = [EmoError('a'), res[1], EmoError('b')]
    out, _ = inf.check_pairs(both, [3, 1, 3], None, ctl.take([0, 1, 4]), [0, None])
    assert out[0] is both[0] and len(out) == 2                                     # both rows failed alike: the leader's error stands


# ------------------------------------------------------------------------------------------------ DrawControls
def test_repeat_and_take_renumber_the_pairs():
    from emo_disentanger_amd import gen_loop as gl
    base = gl.draw_controls('t', 3, 40, [[1], None, [2]], [1.0, 1.1, 1.2], 0.9)
    assert base.guide_arg is None and base.tables().keys() == {'tok_mask', 'mask_of', 'temp_of'} and base.followers() == []
    assert base.with_guidance([0.0, 0.0, 0.0]) is base
    ctl = base.with_guidance([1.5, 0.0, 0.5])
    assert ctl.n == 5 and ctl.bans == [(1,), None, (2,), (1,), (2,)] and ctl.temps == [1.0, 1.1, 1.2, 1.0, 1.2]
    assert ctl.guide_arg == ([0, -1, 2, 0, 2], [3, -1, 4, 3, 4], [1.5, 0.0, 0.5, 1.5, 0.5])
    assert [ctl.guided(r) for r in range(5)] == [True, False, True, True, True] and ctl.followers() == [3, 4]
    tabs = ctl.tables()
    assert tabs['guide_cond'].dtype == np.int32 and tabs['guide_uncond'].tolist() == [3, -1, 4, 3, 4] and tabs['guide_scale'].dtype == np.float32
    rep = ctl.repeat(2)
    assert rep.n == 10 and rep.guide_arg == ([0, 1, -1, -1, 4, 5, 0, 1, 4, 5], [6, 7, -1, -1, 8, 9, 6, 7, 8, 9],
                                             [1.5, 1.5, 0.0, 0.0, 0.5, 0.5, 1.5, 1.5, 0.5, 0.5])
    assert rep.followers() == [6, 7, 8, 9] and rep.bans[6] == (1,) and rep.temp_at(9) == 1.2
    # the streams a later loop takes over: a pair together, in any order; the unguided stream alone; never half a pair
    sub = ctl.take([4, 2])
    assert sub.guide_arg == ([1, 1], [0, 0], [0.5, 0.5]) and sub.followers() == [0] and sub.bans == [(2,), (2,)]
    assert ctl.take([1]).guide_arg is None and ctl.take([1]).tables().keys() == {'temp_of'}
    with pytest.raises(ValueError, match='partner'):
        ctl.take([0, 1])
    with pytest.raises(ValueError, match='partner'):
        ctl.take([0, 0, 3])
    # draw_controls checks pairs it is handed (the loop classes call it on what they are given)
    again = gl.draw_controls('t', 5, 40, ctl.bans, ctl.temps, 0.9, ctl.guide_arg)
    assert again.guide_arg == ctl.guide_arg
    with pytest.raises(ValueError, match='differ in ban, temp or top_p'):
        gl.draw_controls('t', 5, 40, ctl.bans, [1.0, 1.1, 1.2, 1.3, 1.2], 0.9, ctl.guide_arg)
    with pytest.raises(ValueError, match='names one row twice'):
        gl.draw_controls('t', 2, 40, None, 1.2, 0.9, ([0, 0], [0, 0], [1.0, 1.0]))
    with pytest.raises(ValueError, match='for 5 inputs'):
        gl.draw_controls('t', 5, 40, None, 1.2, 0.9, ([0, 0], [1, 1], [1.0, 1.0]))


class _Loop:
    """GrammarLoop on host tensors: ptr() is the one thing of block_set that needs the device."""

    def __new__(cls, monkeypatch):
        from emo_disentanger_amd import gen_loop as gl, ops
        monkeypatch.setattr(ops, 'ptr', lambda t: None if t is None else t.data_ptr())
        loop = gl.GrammarLoop()
        loop.dev, loop.seq = 'cpu', torch.zeros(5, 16, dtype=torch.int64)
        return loop


def test_a_loop_owns_the_guidance_tables_and_only_the_lock_step_kind_takes_them(monkeypatch):
    from emo_disentanger_amd import gen_loop as gl, ops
    from emo_disentanger_amd._lib import EmoError
    ctl = gl.draw_controls('t', 3, 40, None, 1.2, 0.9).with_guidance([1.5, 0.0, 0.5])
    loop = _Loop(monkeypatch)
    loop._build_block(ops.GRAMMAR_ACC, False, ctl, n_rows=5, n_token=40, ld_u=5, temperature=1.2, top_p=0.9)
    a, t = loop._gargs, loop.control_tables
    assert sorted(t) == sorted(NEW) and all(getattr(a, k) == t[k].data_ptr() and loop._gheld[k] is t[k] for k in NEW)
    assert a.tok_mask is None and a.temp_of is None and t['guide_cond'].tolist() == [0, -1, 2, 0, 2] and t['guide_scale'].tolist() == [1.5, 0.0, 0.5, 1.5, 0.5]
    for kind in (ops.GRAMMAR_ACC_QUEUE, ops.GRAMMAR_ACC_WINDOW, ops.GRAMMAR_TXL):
        with pytest.raises(EmoError, match='guidance pairs'):
            _Loop(monkeypatch)._build_block(kind, False, ctl, n_rows=5, n_token=40, ld_u=5, temperature=1.2, top_p=0.9)
    # without guidance every new field stays NULL
    loop = _Loop(monkeypatch)
    loop._build_block(ops.GRAMMAR_ACC, False, gl.draw_controls('t', 5, 40, None, 1.2, 0.9), n_rows=5, n_token=40, ld_u=5, temperature=1.2, top_p=0.9)
    assert all(getattr(loop._gargs, k) is None for k in NEW) and loop.control_tables == {}


# ------------------------------------------------------------------------------------------------ command line
def test_the_guidance_flag_needs_the_device_path():
    from emo_disentanger_amd import inference as inf
    base = ['-m', 'performer', '-c', 'conf.yaml', '-r', 'functional', '-i', 'params.pt', '-o', 'out']
    assert inf.parse_args(base).guidance is None and inf.parse_args(base + ['--device']).guidance is None
    assert inf.parse_args(base + ['--device', '--guidance', '1.5']).guidance == 1.5
    assert inf.parse_args(base + ['--device', '--guidance', '2', '--window', 'rebase', '--best-of', '2']).guidance == 2.0
    assert inf.parse_args(base + ['--device', '--guidance', '0', '--slots', '4']).guidance == 0.0      # no piece is guided: the queue may run
    for bad in (['--guidance', '1.5'], ['--device', '--guidance', '-1'], ['--device', '--guidance', 'inf'], ['--device', '--guidance', 'nan'],
                ['--device', '--guidance', '1.5', '--slots', '4'], ['--device', '--guidance', '1.5', '--window', 'device']):
        with pytest.raises(SystemExit):
            inf.parse_args(base + bad)
