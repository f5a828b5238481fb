"""CPU: the host side of stage-2 generation from a queue (emo_grammar_step, kind ACC_QUEUE; emo_favor_state_reset): the refusals of the new kind
and of the new entry, which need no GPU, the ctypes mirror, the slots= argument of generate_accompaniments and the --slots flag, and
queue_plan (stage1_inference's, which plans this queue too) on hand-made job_steps."""
import ctypes
from types import SimpleNamespace

import pytest

ACC_QUEUE = 4


def _args(**kw):
    """A block that passes every host check of kind ACC_QUEUE (pointer fields: small fake addresses — validation never dereferences them, and no
    refusal below gets as far as the launch), with the fields of `kw` changed."""
    from emo_disentanger_amd import _lib
    a = _lib.GrammarStep()
    for name, ctype in _lib.GrammarStep._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.kind, a.n_rows, a.n_token, a.n_u, a.ld_u, a.ld_seq, a.max_len, a.n_jobs, a.mem_rows = ACC_QUEUE, 3, 327, 8, 11, 64, 32, 11, 32
    a.temperature, a.top_p = 1.2, 0.9
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('kw, what', [
    (dict(slot_job=None), 'null pointer'), (dict(queue_head=None), 'null pointer'), (dict(mem_lens=None), 'null pointer'),
    (dict(row_reset=None), 'null pointer'), (dict(seg_out=None), 'null pointer'), (dict(tok_out=None), 'null pointer'),
    (dict(segs=None), 'null pointer'), (dict(lead_off=None), 'null pointer'), (dict(running=None), 'null pointer'),
    (dict(n_jobs=0), 'bad sizes'), (dict(n_jobs=12), 'bad sizes'), (dict(mem_rows=0), 'bad sizes'), (dict(max_len=0), 'bad sizes'),
    (dict(n_u=0), 'bad sizes'), (dict(n_rows=0), 'bad sizes'),
    (dict(n_token=2000), 'V must be <= 1024 (got 2000)'), (dict(temperature=0.0), 'temperature must be > 0'),
])
def test_acc_queue_refuses_bad_arguments_without_a_gpu_and_names_its_kind(kw, what):
    from emo_disentanger_amd import _lib
    assert _lib.GRAMMAR_ACC_QUEUE == ACC_QUEUE
    assert _lib.lib.emo_grammar_step(ctypes.byref(_args(**kw)), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert msg.startswith('emo_grammar_step[acc_queue]: ') and what in msg, msg


def test_acc_queue_ignores_the_fields_of_the_other_kinds_and_allows_more_slots_than_jobs():
    # the windowed kind's and TXL's fields NULL / 0, job_steps and the score tables NULL, 16 slots for 11 jobs: the block gets as far as its next
    # refusal, a size of its own
    from emo_disentanger_amd import _lib
    a = _args(rows=None, win_tok=None, win_seg=None, window=0, key_temperature=0.0, job_steps=None, tok_logp=None, tok_rank=None, tok_entropy=None,
              n_rows=16, n_u=0)
    assert _lib.lib.emo_grammar_step(ctypes.byref(a), None) == -1
    assert _lib.lib.emo_last_error().decode() == 'emo_grammar_step[acc_queue]: bad sizes'


def test_the_mirror_has_the_library_size_and_row_reset_stands_before_the_scores():
    from emo_disentanger_amd import _lib
    assert _lib.lib.emo_grammar_step_size() == ctypes.sizeof(_lib.GrammarStep)
    names = [f[0] for f in _lib.GrammarStep._fields_]
    assert names[-4:] == ['row_reset', 'tok_logp', 'tok_rank', 'tok_entropy']
    assert _lib.lib.emo_grammar_step(ctypes.byref(_args(kind=5)), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert msg.startswith('emo_grammar_step: ') and 'kind 5' in msg


@pytest.mark.parametrize('kw, what', [
    (dict(table=None), 'null pointer'), (dict(flags=None), 'null pointer'),
    (dict(layers=0), 'bad sizes'), (dict(rows=0), 'bad sizes'), (dict(rows=-2), 'bad sizes'), (dict(s_row=0), 'bad sizes'), (dict(z_row=-4), 'bad sizes'),
    (dict(s_row=1022), 'multiples of 4'), (dict(z_row=6), 'multiples of 4'), (dict(layers=70000), 'grid too large'),
])
def test_favor_state_reset_refusals_without_a_gpu(kw, what):
    from emo_disentanger_amd import _lib
    v = dict(table=0x1000, layers=3, rows=5, s_row=1024, z_row=32, flags=0x2000)
    v.update(kw)
    assert _lib.lib.emo_favor_state_reset(v['table'], v['layers'], v['rows'], v['s_row'], v['z_row'], v['flags'], None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert msg.startswith('emo_favor_state_reset: ') and what in msg, msg


def _fake_model():
    m = SimpleNamespace(training=False, n_token=327, calls=[])
    m.eval = lambda: m.calls.append('eval')
    m.train = lambda mode=True: m.calls.append(('train', mode))
    return m


def test_slots_argument_of_generate_accompaniments(monkeypatch):
    from emo_disentanger_amd import inference as inf
    leads, primers = [[[5, 6]], [[7]], [[8, 9]]], [[1], [2], [3]]
    for bad in (0, -1, 'x'):
        with pytest.raises(ValueError, match='slots must be'):
            inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, slots=bad)
    # the existing checks come first, in the order they have
    with pytest.raises(ValueError, match='window must be'):
        inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, slots=0, window='gpu')
    with pytest.raises(ValueError, match='inadmissibles'):
        inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, slots=0, inadmissibles=[1])
    with pytest.raises(ValueError, match='inadmissibles'):
        inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, slots=2, inadmissibles=[1])      # refused on the queue path too
    with pytest.raises(ValueError, match='best_of must be at least 1'):
        inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, slots=0, best_of=0)
    with pytest.raises(ValueError, match='slots must be at least 1'):
        inf.AccompanimentQueue(None, {}, {}, leads, primers, 0)
    built = []

    class Fake:
        bound = 48

        def __init__(self, model, e2i, i2e, lead_sheets, primers, *a, **kw):
            built.append((type(self).__name__, a, len(lead_sheets), kw['seed'], kw['scores']))
            self.n = len(lead_sheets)

        def run(self, use_graph=True):
            pass

        def results(self, *a, **kw):
            return [[1, 2]] * self.n

    monkeypatch.setattr(inf, 'AccompanimentLoop', type('Loop', (Fake,), {}))
    monkeypatch.setattr(inf, 'AccompanimentQueue', type('Queue', (Fake,), {}))
    res, _ = inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, seed=4)
    assert built == [('Loop', (), 3, 4, False)] and res == [[1, 2]] * 3                 # slots=None: the lock-step loop, as before
    res, _ = inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, seed=5, slots=2)
    assert built[-1] == ('Queue', (2,), 3, 5, False) and len(res) == 3                    # every lead sheet is a job of ONE queue of 2 slots
    res, _ = inf.generate_accompaniments(_fake_model(), {}, {}, leads, primers, seed=5, slots=16)
    assert built[-1] == ('Queue', (16,), 3, 5, False)                                     # more slots than jobs: still the queue


def test_slots_flag():
    from emo_disentanger_amd import inference as inf
    base = ['-m', 'performer', '-c', 'conf.yaml', '-r', 'functional', '-i', 'params.pt', '-o', 'out']
    assert inf.parse_args(base).slots is None
    assert inf.parse_args(base + ['--device', '--slots', '8', '--best-of', '2', '--window', 'device']).slots == 8
    for bad in (['--slots', '4'], ['--device', '--slots', '0']):
        with pytest.raises(SystemExit):
            inf.parse_args(base + bad)


def test_queue_plan_is_stage_ones_and_plans_hand_made_job_steps():
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    assert not hasattr(inf, 'queue_plan') or inf.queue_plan is s1.queue_plan
    # job_steps = the tokens the model was fed for a job: its prompt, its accepted words and its injected bars.  11 jobs through 3 slots: slot A
    # 9 + 4 + 12 + 6 = 31, slot B 14 + 7 + 5 + 8 = 34, slot C 20 + 3 + 10 = 33; the first launch only admits
    steps = [9, 14, 20, 4, 12, 7, 3, 5, 10, 6, 8]
    launches, occ = s1.queue_plan(steps, 3)
    assert launches == 35 and occ == sum(steps) / float(35 * 3)
    # a job that reached the window holds its slot for W launches and no longer; one closed before the run holds none
    assert s1.queue_plan([48, 0, 5, 5], 2) == (49, 58 / 98.0)
    # at least as many slots as jobs: the longest job decides
    assert s1.queue_plan(steps, 16)[0] == 21
