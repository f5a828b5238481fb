"""CPU: the host side of stage-1 generation from a queue (emo_grammar_step, kind TXL_QUEUE): queue_plan on hand-checked cases, the slots=
argument of generate_lead_sheets and the --slots flag."""
from types import SimpleNamespace

import pytest


def test_queue_plan_on_hand_checked_cases():
    from emo_disentanger_amd.stage1_inference import queue_plan
    # The first launch admits; a job of s steps then holds its slot for s launches and its successor starts in the launch it ends in.
    # more slots than jobs: both jobs start at launch 1, the longer one ends 5 launches later
    assert queue_plan([3, 5], 4) == (6, 8 / 24.0)
    # one slot: the jobs follow each other without a gap
    assert queue_plan([3, 2, 4], 1) == (10, 9 / 10.0)
    # equal lengths: two full rounds of three
    assert queue_plan([4] * 6, 3) == (9, 24 / 27.0)
    # one long job among short ones: slot A runs 2 + 10, slot B runs 2 + 2 + 2 + 2 and then idles
    assert queue_plan([2, 2, 10, 2, 2, 2], 2) == (13, 20 / 26.0)
    # the long job last: slot A runs 2 + 2 + 2 and idles, slot B runs 2 + 2 + 10
    assert queue_plan([2, 2, 2, 2, 2, 10], 2) == (15, 20 / 30.0)
    # a job that was closed before the run holds no slot
    assert queue_plan([0, 3], 1) == (4, 3 / 4.0)
    assert queue_plan([], 3) == (0, 0.0)
    with pytest.raises(ValueError):
        queue_plan([1, 2], 0)
    with pytest.raises(ValueError):
        queue_plan([1, -2], 2)


@pytest.mark.parametrize('steps,slots', [([7, 1, 3, 9, 2, 2, 5], 3), ([5] * 9, 4), ([1], 1), ([3, 3], 8), (list(range(1, 40)), 5)])
def test_queue_plan_occupancy_is_the_share_of_rows_that_carried_a_token(steps, slots):
    from emo_disentanger_amd.stage1_inference import queue_plan
    launches, occ = queue_plan(steps, slots)
    assert occ == sum(steps) / float(launches * slots) and 0.0 < occ <= 1.0
    # no schedule beats the two lower bounds, and handing the head of the queue to the first free slot stays within one job of them
    assert launches - 1 >= max(max(steps), -(-sum(steps) // slots))
    assert launches - 1 <= sum(steps) // slots + max(steps)


def _fake_model():
    m = SimpleNamespace(training=False, calls=[])
    m.eval = lambda: m.calls.append('eval')
    m.train = lambda mode=True: m.calls.append(('train', mode))
    return m


def test_slots_argument_of_generate_lead_sheets(monkeypatch):
    from emo_disentanger_amd import stage1_inference as s1
    for bad in (0, -3):
        with pytest.raises(ValueError, match='slots must be at least 1'):
            s1.generate_lead_sheets(None, {}, {}, [['Emotion_Q1']], slots=bad)       # refused before the model is looked at
    with pytest.raises(ValueError, match='slots must be at least 1'):
        s1.LeadSheetQueue(None, {}, {}, [['Emotion_Q1']], 0)
    with pytest.raises(ValueError, match='step must be one of'):
        s1.LeadSheetQueue(None, {}, {}, [['Emotion_Q1']], 2, step='one-launch')
    built = []

    class Fake:
        def __init__(self, model, e2i, i2e, primers, *a, **kw):
            built.append((type(self).__name__, a, len(primers), kw['seed'], kw['step'], kw['scores']))
            self.n = len(primers)

        def run(self, use_graph=True):
            pass

        def results(self):
            return [[1, 2]] * self.n

    monkeypatch.setattr(s1, 'LeadSheetLoop', type('Loop', (Fake,), {}))
    monkeypatch.setattr(s1, 'LeadSheetQueue', type('Queue', (Fake,), {}))
    primers = [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Q3']]
    res, _ = s1.generate_lead_sheets(_fake_model(), {}, {}, primers, seed=4)
    assert built == [('Loop', (), 3, 4, 'chain', False)] and res == [[1, 2]] * 3          # slots=None: the lock-step loop, as before
    res, _ = s1.generate_lead_sheets(_fake_model(), {}, {}, primers, seed=4, slots=None, step='one_launch')
    assert built[-1] == ('Loop', (), 3, 4, 'one_launch', False)
    res, _ = s1.generate_lead_sheets(_fake_model(), {}, {}, primers, seed=5, slots=2)
    assert built[-1] == ('Queue', (2,), 3, 5, 'chain', False) and len(res) == 3           # every primer is a job of ONE queue of 2 slots


def test_slots_flag():
    from emo_disentanger_amd import stage1_inference as s1
    base = ['-c', 'conf.yaml', '-r', 'functional', '-m', 'lead_sheet']
    assert s1.parse_args(base).slots is None
    assert s1.parse_args(base + ['--slots', '8', '--step', 'one-launch', '--best-of', '2']).slots == 8
    for bad in (['--slots', '0'], ['--slots', '4', '--exact']):
        with pytest.raises(SystemExit):
            s1.parse_args(base + bad)
    assert s1.MEM_FULL == 5 and s1.RUNNING == 0
