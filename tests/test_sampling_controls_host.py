"""CPU: the host side of the per-job sampling controls of the device draw (emo_grammar_step_t: tok_mask / n_masks / mask_of / temp_of /
top_p_of): the packing of the ban rows, tempo_ban / key_ban, every refusal of generate_*(banned=, temp=, top_p=), the input -> job mapping under
best_of and slots, the ctypes mirror, and that a loop built without controls leaves every new field NULL."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

NEW = ['tok_mask', 'n_masks', 'mask_of', 'temp_of', 'top_p_of']


def _bits(mask_row, V):
    """the banned ids a packed row names, read back by the layout of emo_hip.h: bit v & 31 of word v >> 5"""
    return [v for v in range(V) if (int(mask_row[v >> 5]) >> (v & 31)) & 1]


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize('V', [31, 32, 33, 64, 65, 327, 1024])
def test_masks_pack_as_bit_v_and_31_of_word_v_shift_5(V):
    from emo_disentanger_amd import gen_loop as gl
    rs = np.random.RandomState(V)
    edge = sorted({0, 30, 31, 32, 33, 63, 64, V - 2, V - 1} & set(range(V)))
    some = sorted(rs.choice(V, size=V // 3, replace=False).tolist())
    mask, mask_of = gl.pack_token_masks([edge, None, some, [V - 1]], V)
    assert mask.dtype == np.uint32 and mask.shape == (3, (V + 31) // 32) and gl.mask_words(V) == (V + 31) // 32
    assert mask_of.dtype == np.int32 and mask_of.tolist() == [0, -1, 1, 2]
    assert _bits(mask[0], V) == edge and _bits(mask[1], V) == some and _bits(mask[2], V) == [V - 1]
    # the last id alone: one bit, in the last word; nothing at or beyond V is ever set
    assert int(mask[2, -1]) == 1 << ((V - 1) & 31) and not mask[2, :-1].any()
    for row in mask:
        assert int(row[-1]) >> (((V - 1) & 31) + 1) == 0


def test_equal_masks_are_stored_once_and_streams_without_a_ban_get_minus_one():
    from emo_disentanger_amd import gen_loop as gl
    mask, mask_of = gl.pack_token_masks([[5, 3], None, (3, 5, 5), [], [7], np.array([5, 3]), [7]], 40)
    assert mask_of.tolist() == [0, -1, 0, -1, 1, 0, 1] and mask.shape == (2, 2)
    assert _bits(mask[0], 40) == [3, 5] and _bits(mask[1], 40) == [7]
    mask, mask_of = gl.pack_token_masks([None, None], 40)
    assert mask.shape == (0, 2) and mask_of.tolist() == [-1, -1]
    ctl = gl.draw_controls('t', 3, 40, [[1], None, [1]], 1.2, 0.9)
    assert sorted(ctl.tables()) == ['mask_of', 'tok_mask'] and len(ctl.tables()['tok_mask']) == 1
    assert gl.draw_controls('t', 3, 40, None, 1.2, 0.9).tables() == {}
    tabs = gl.draw_controls('t', 3, 40, None, [1.0, 1.1, 1.2], 0.9).tables()
    assert list(tabs) == ['temp_of'] and tabs['temp_of'].dtype == np.float32 and tabs['temp_of'].tolist() == [np.float32(x) for x in (1.0, 1.1, 1.2)]
    assert list(gl.draw_controls('t', 3, 40, None, 1.0, (0.5, 0.9, 1.0)).tables()) == ['top_p_of']


# ------------------------------------------------------------------------------------------------ the two helpers
VOCAB = ['Emotion_Q1', 'Key_C', 'Key_a', 'Key_G', 'Tempo_50', 'Tempo_89', 'Tempo_90', 'Tempo_110', 'Tempo_130', 'Tempo_131', 'Tempo_200',
         'Tempo_Conti', 'Conti_Tempo_300', 'Beat_0', 'Note_Pitch_110', 'Bar_None', 'PAD_None']


def test_tempo_ban_is_the_references_rule():
    from emo_disentanger_amd import inference as inf
    e2i = {e: i for i, e in enumerate(VOCAB)}

    def rule(tempo, tolerance):
        """The reference's construct_inadmissible_set, restated: Tempo and not Conti in the key, trailing integer further than tolerance."""
        out = []
        for k, i in e2i.items():
            if 'Tempo' in k and 'Conti' not in k and abs(int(k.split('_')[-1]) - tempo) > tolerance:
                out.append(i)
        return out

    for tempo, tol in ((110, 20), (110, 0), (60, 20), (200, 75), (110, 1000)):
        kw = {} if tol == 20 else {'tolerance': tol}
        assert sorted(inf.tempo_ban(e2i, tempo, **kw)) == sorted(rule(tempo, tol))
    names = [VOCAB[i] for i in inf.tempo_ban(e2i, 110)]
    assert sorted(names) == ['Tempo_131', 'Tempo_200', 'Tempo_50', 'Tempo_89']          # 90 and 130 are at the tolerance: allowed
    assert inf.tempo_ban(e2i, 110, 1000) == []


def test_key_ban_is_every_key_but_the_one():
    from emo_disentanger_amd import stage1_inference as s1
    e2i = {e: i for i, e in enumerate(VOCAB)}
    assert [VOCAB[i] for i in s1.key_ban(e2i, 'Key_a')] == ['Key_C', 'Key_G']
    for bad in ('Key_X', 'Tempo_110', 'a'):
        with pytest.raises(ValueError, match='key_ban'):
            s1.key_ban(e2i, bad)


# ------------------------------------------------------------------------------------------------ refusals
def _fake_model(V=40):
    m = SimpleNamespace(training=False, n_token=V, vocab_size=V, calls=[])
    m.eval = lambda: m.calls.append('eval')
    m.train = lambda mode=True: m.calls.append(('train', mode))
    return m


BAD = [
    (dict(banned=[40]), 'outside'), (dict(banned=[[1], [-1], None]), 'outside'), (dict(banned=[None, None, [3, 1024]]), 'outside'),
    (dict(banned=list(range(40))), 'bans every token'), (dict(banned=[None, list(range(40)) * 2, None]), 'bans every token'),
    (dict(banned=[[1], [2]]), 'entries for 3 inputs'), (dict(banned=[[1], None, None, None]), 'entries for 3 inputs'),
    (dict(banned=[1, [2], None]), 'mixes'),
    (dict(temp=0.0), 'temp must be > 0'), (dict(temp=-1.0), 'temp must be > 0'), (dict(temp=[1.0, 0.0, 1.0]), 'temp must be > 0'),
    (dict(temp=[1.0, 1.0]), 'temp has 2 entries for 3 inputs'), (dict(temp=float('nan')), 'temp must be > 0'),
    (dict(top_p=0.0), r'top_p must be in \(0, 1\]'), (dict(top_p=1.5), r'top_p must be in \(0, 1\]'),
    (dict(top_p=[0.9, 0.9, 1.01]), r'top_p must be in \(0, 1\]'), (dict(top_p=[0.9] * 4), 'top_p has 4 entries for 3 inputs'),
]


@pytest.mark.parametrize('kw, what', BAD)
def test_both_generators_refuse_bad_controls_before_anything_is_allocated(monkeypatch, kw, what):
    from emo_disentanger_amd import inference as inf, stage1_inference as s1

    def never(*a, **k):
        raise AssertionError('a loop was built')

    for mod, names in ((inf, ('AccompanimentLoop', 'AccompanimentQueue')), (s1, ('LeadSheetLoop', 'LeadSheetQueue'))):
        for name in names:
            monkeypatch.setattr(mod, name, never)
    for extra in ({}, {'slots': 2}, {'best_of': 2}):
        with pytest.raises(ValueError, match=what):
            inf.generate_accompaniments(_fake_model(), {}, {}, [[[5, 6]], [[7]], [[8, 9]]], [[1], [2], [3]], **kw, **extra)
        with pytest.raises(ValueError, match=what):
            s1.generate_lead_sheets(_fake_model(), {}, {}, [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Q3']], **kw, **extra)
    # the check itself, which the loop classes run on what they are handed before they allocate
    from emo_disentanger_amd import gen_loop as gl
    with pytest.raises(ValueError, match=what):
        gl.draw_controls('x', 3, 40, kw.get('banned'), kw.get('temp', 1.2), kw.get('top_p', 0.9))


def test_inadmissibles_stays_refused_and_the_docstring_names_banned():
    from emo_disentanger_amd import inference as inf
    with pytest.raises(ValueError, match='`inadmissibles` is not supported by the device grammar'):
        inf.generate_accompaniments(_fake_model(), {}, {}, [[[5]]], [[1]], inadmissibles=[1], banned=[2])
    assert 'banned' in inf.generate_accompaniments.__doc__ and 'inadmissibles' in inf.generate_accompaniments.__doc__


# ------------------------------------------------------------------------------------------------ input -> job mapping
@pytest.mark.parametrize('slots', [None, 2])
@pytest.mark.parametrize('best_of', [1, 2, 3])
def test_every_candidate_and_job_of_an_input_inherits_its_controls(monkeypatch, best_of, slots):
    from emo_disentanger_amd import inference as inf, scoring, stage1_inference as s1
    built = []

    class Fake:
        bound = 48

        def __init__(self, model, e2i, i2e, *inputs, **kw):
            built.append((type(self).__name__, inputs, kw))
            self.n = len(inputs[0])
            self.params = SimpleNamespace(cpu=lambda: SimpleNamespace(numpy=lambda: np.ones((self.n, 8), dtype=np.int32)))

        def run(self, use_graph=True):
            pass

        def results(self, *a, **kw):
            return [[1, 2]] * self.n

    for mod, names in ((inf, ('AccompanimentLoop', 'AccompanimentQueue')), (s1, ('LeadSheetLoop', 'LeadSheetQueue'))):
        for name in names:
            monkeypatch.setattr(mod, name, type(name, (Fake,), {}))
    monkeypatch.setattr(scoring, 'lead_sheet_candidate_scores', lambda model, cands, plens: [0.0] * len(cands))
    monkeypatch.setattr(scoring, 'candidate_scores', lambda model, e2i, cands, max_len: [0.0] * len(cands))
    ctl = dict(banned=[[9, 3, 3], None, (4,)], temp=[1.0, 1.1, 1.2], top_p=[0.5, 0.9, 1.0])
    flags = dict(best_of=best_of, slots=slots)
    inf.generate_accompaniments(_fake_model(), {}, {}, [[[5, 6]], [[7]], [[8, 9]]], [[1], [2], [3]], **ctl, **flags)
    s1.generate_lead_sheets(_fake_model(), {}, {}, [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Q3']], **ctl, **flags)
    rep = lambda v: [x for x in v for _ in range(best_of)]                           # noqa: E731  (candidate c of input i is stream i * N + c)
    for name, inputs, kw in built:
        assert name.endswith('Queue') == (slots is not None)
        assert len(inputs[0]) == 3 * best_of
        assert kw['banned'] == rep([(3, 9), None, (4,)]) and kw['temp'] == rep([1.0, 1.1, 1.2]) and kw['top_p'] == rep([0.5, 0.9, 1.0])
    built.clear()
    # one sequence of ids holds for every input; scalars stay scalars
    inf.generate_accompaniments(_fake_model(), {}, {}, [[[5, 6]], [[7]], [[8, 9]]], [[1], [2], [3]], banned=[7, 5], temp=1.3, **flags)
    s1.generate_lead_sheets(_fake_model(), {}, {}, [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Q3']], banned=np.array([7, 5]), top_p=0.8, **flags)
    assert [kw['banned'] for _, _, kw in built] == [[(5, 7)] * (3 * best_of)] * 2
    assert built[0][2]['temp'] == 1.3 and built[0][2]['top_p'] == 0.9 and built[1][2]['temp'] == 1.2 and built[1][2]['top_p'] == 0.8
    built.clear()
    inf.generate_accompaniments(_fake_model(), {}, {}, [[[5, 6]], [[7]], [[8, 9]]], [[1], [2], [3]], **flags)
    assert built[0][2]['banned'] == [None] * (3 * best_of) and built[0][2]['temp'] == 1.2


def test_controls_of_a_subset_and_of_repeats():
    from emo_disentanger_amd import gen_loop as gl
    ctl = gl.draw_controls('t', 3, 40, [[1], None, [2]], [1.0, 1.1, 1.2], 0.9)
    sub = ctl.take([2, 0])                                                          # the streams a windowed loop takes over
    assert sub.n == 2 and sub.bans == [(2,), (1,)] and sub.temps == [1.2, 1.0] and sub.top_ps is None and sub.top_p_at(1) == 0.9
    assert ctl.repeat(2).bans == [(1,), (1,), None, None, (2,), (2,)] and ctl.repeat(2).temp_at(3) == 1.1


# ------------------------------------------------------------------------------------------------ the block
def test_the_mirror_holds_the_new_fields_in_front_of_row_reset_and_the_scores():
    from emo_disentanger_amd import _lib
    G = _lib.GrammarStep
    names = [f[0] for f in G._fields_]
    at = names.index('job_steps')
    assert names[at + 1:] == NEW + ['row_reset', 'tok_logp', 'tok_rank', 'tok_entropy']        # (row_reset and the scores stay the tail)
    assert _lib.lib.emo_grammar_step_size() == ctypes.sizeof(G)
    # the C layout: eight-byte fields, one after another, the struct ending behind tok_entropy
    off = G.job_steps.offset
    for k in names[at + 1:]:
        off += 8
        assert getattr(G, k).offset == off and getattr(G, k).size == 8, k
    assert off + 8 == _lib.lib.emo_grammar_step_size()


class _Loop:
    """GrammarLoop on host tensors: ptr() is the one thing of block_set that needs the device."""

    def __new__(cls, monkeypatch):
        from emo_disentanger_amd import gen_loop as gl, ops
        monkeypatch.setattr(ops, 'ptr', lambda t: None if t is None else t.data_ptr())
        loop = gl.GrammarLoop()
        loop.dev, loop.seq = 'cpu', torch.zeros(4, 16, dtype=torch.int64)
        return loop


def test_a_loop_without_controls_leaves_every_new_field_null(monkeypatch):
    from emo_disentanger_amd import gen_loop as gl, ops
    for controls in (None, gl.draw_controls('t', 4, 40, None, 1.2, 0.9)):
        loop = _Loop(monkeypatch)
        loop._build_block(ops.GRAMMAR_ACC, False, controls, n_rows=4, n_token=40, ld_u=4, temperature=1.2, top_p=0.9)
        a = loop._gargs
        assert a.tok_mask is None and a.mask_of is None and a.temp_of is None and a.top_p_of is None and a.n_masks == 0
        assert loop.control_tables == {} and not any(k in loop._gheld for k in NEW)


def test_a_loop_with_controls_owns_their_tables_once(monkeypatch):
    from emo_disentanger_amd import gen_loop as gl, ops
    loop = _Loop(monkeypatch)
    ctl = gl.draw_controls('t', 4, 40, [[1, 39], None, [39, 1], [2]], [1.0, 1.1, 1.2, 1.3], 0.9)
    loop._build_block(ops.GRAMMAR_ACC, False, ctl, n_rows=4, n_token=40, ld_u=4, temperature=ctl.temp, top_p=ctl.top_p)
    a, t = loop._gargs, loop.control_tables
    assert a.n_masks == 2 and sorted(t) == ['mask_of', 'temp_of', 'tok_mask'] and a.top_p_of is None
    assert a.tok_mask == t['tok_mask'].data_ptr() and a.mask_of == t['mask_of'].data_ptr() and a.temp_of == t['temp_of'].data_ptr()
    assert all(loop._gheld[k] is t[k] for k in t)
    assert t['tok_mask'].dtype == torch.int32 and t['tok_mask'].shape == (2, 2) and t['mask_of'].tolist() == [0, -1, 0, 1]
    assert _bits(t['tok_mask'].numpy().view(np.uint32)[0], 40) == [1, 39]
    assert a.temperature == 1.0 and loop.controls is ctl


def test_block_set_refuses_a_mask_row_outside_the_table(monkeypatch):
    from emo_disentanger_amd import ops
    monkeypatch.setattr(ops, 'ptr', lambda t: None if t is None else t.data_ptr())
    mask = torch.zeros(2, 2, dtype=torch.int32)
    for bad in ([0, 2, -1, 1], [0, -2, -1, 1], [0, 1000, 0, 0]):
        with pytest.raises(AssertionError, match='mask_of'):
            ops.block_set(ops.GrammarStep(), {}, n_token=40, ld_u=4, n_masks=2, tok_mask=mask, mask_of=torch.tensor(bad, dtype=torch.int32))
    args = ops.GrammarStep()
    ops.block_set(args, {}, n_token=40, ld_u=4, n_masks=2, tok_mask=mask, mask_of=torch.tensor([0, -1, 1, 1], dtype=torch.int32))
    assert args.mask_of is not None
    with pytest.raises(AssertionError, match='mask_of'):                                  # without a table every row is outside it
        ops.block_set(ops.GrammarStep(), {}, n_token=40, ld_u=4, mask_of=torch.tensor([0, -1, -1, -1], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ command lines
def test_tempo_and_key_flags():
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    base = ['-m', 'performer', '-c', 'conf.yaml', '-r', 'functional', '-i', 'params.pt', '-o', 'out']
    a = inf.parse_args(base)
    assert a.tempo is None and a.tempo_tolerance is None
    a = inf.parse_args(base + ['--device', '--tempo', '90'])
    assert a.tempo == 90 and a.tempo_tolerance == 20
    assert inf.parse_args(base + ['--device', '--slots', '4', '--tempo', '90', '--tempo-tolerance', '5']).tempo_tolerance == 5
    assert inf.parse_args(base + ['--tempo', '120']).tempo == 120                    # the host loop takes it as inadmissibles
    for bad in (['--tempo-tolerance', '5'], ['--tempo', '90', '--tempo-tolerance', '-1']):
        with pytest.raises(SystemExit):
            inf.parse_args(base + bad)
    base = ['-c', 'conf.yaml', '-r', 'functional', '-m', 'lead_sheet']
    assert s1.parse_args(base).key is None and s1.parse_args(base + ['--key', 'Key_C', '--slots', '4']).key == 'Key_C'
    for bad in (['--key', 'Key_C', '--exact'], ['--key', 'C']):
        with pytest.raises(SystemExit):
            s1.parse_args(base + bad)
    with pytest.raises(SystemExit):
        s1.parse_args(['-c', 'conf.yaml', '-r', 'remi', '-m', 'lead_sheet', '--key', 'Key_C'])
