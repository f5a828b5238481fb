"""Host: kept bars (keep=) in the stage-2 grammar.  inference._Stream._open_bar is the rule the device launch is held to; here it is held to
sequences written out by hand, keep=None to the stream as it was and to the reference's recorded runs, and the helpers around it (check_keep,
pack_keep, bars_of, parse_reroll, the block setter's checks) to their definitions."""
import json
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(__file__), 'golden')
GEN = json.load(open(os.path.join(G, 'generate.json')))
E2I = {e: i for i, e in enumerate(GEN['events'])}
I2E = {i: e for e, i in E2I.items()}
LS, TF, EOS, PAD = E2I['Track_LeadSheet'], E2I['Track_Full'], E2I['EOS_None'], E2I['PAD_None']
LEAD = [list(b) for b in GEN['lead']]                # three bars
PRIMER = list(GEN['primer'])
A, B_, C = E2I['Note_Octave_4'], E2I['Chord_I_M'], E2I['Note_Degree_1']
BEAT = lambda k: E2I['Beat_%d' % k]                 # noqa: E731


def stream(keep, lead=LEAD, max_bars=None, max_events=1000):
    from emo_disentanger_amd import inference as inf
    return inf._Stream(E2I, lead, PRIMER, max_bars, keep, max_events)


def offer(s, words, max_events=1000, skip_check=False):
    out = []
    for w in words:
        assert not s.done
        out.append(s.offer(w, E2I, I2E, skip_check, max_events))
    return out


def head(j):
    """What opening bar j appends behind a Track_LeadSheet, with its segments."""
    return LEAD[j] + [TF], [0] * len(LEAD[j]) + [1]


def test_a_kept_middle_bar_is_written_when_the_bar_before_it_closes():
    s = stream([None, [A, BEAT(9), B_], None])
    h0, g0 = head(0)
    assert s.generated == PRIMER + [LS] + h0 and not s.done
    assert offer(s, [BEAT(4), A, LS]) == [True, True, True]
    h1, g1 = head(1)
    h2, g2 = head(2)
    want = PRIMER + [LS] + h0 + [BEAT(4), A, LS] + h1 + [A, BEAT(9), B_, LS] + h2
    assert s.generated == want
    assert s.seg == [0] * (len(PRIMER) + 1) + g0 + [1, 1, 0] + g1 + [1, 1, 1, 0] + g2
    # the kept Beat_9 set no position: bar 2 starts at 0; two bars are closed, nothing is done
    assert (s.generated_bars, s.cur_pos, s.failed_cnt, s.done) == (2, 0, 0, False)
    assert offer(s, [BEAT(2), LS]) == [True, True] and s.done and s.generated_bars == 3
    assert s.result() == want + [BEAT(2)]


def test_two_consecutive_kept_bars_chain_and_a_kept_last_bar_ends_in_eos_and_done():
    s = stream([None, [A], [B_, C]])
    h0, g0 = head(0)
    h1, g1 = head(1)
    h2, g2 = head(2)
    assert offer(s, [C, LS]) == [True, True]
    want = PRIMER + [LS] + h0 + [C, LS] + h1 + [A, LS] + h2 + [B_, C, EOS]
    assert s.generated == want and s.done and not s.stuck
    # (offer's end-of-piece branch appends no segment for EOS, and counts no bar for it)
    assert s.seg == [0] * (len(PRIMER) + 1) + g0 + [1, 0] + g1 + [1, 0] + g2 + [1, 1]
    assert s.generated_bars == 2 and s.result() == want[:-1]


def test_a_kept_first_bar_and_a_kept_run_of_first_bars_are_in_the_row_from_the_start():
    h0, g0 = head(0)
    h1, g1 = head(1)
    h2, g2 = head(2)
    s = stream([[A, B_]])
    assert s.generated == PRIMER + [LS] + h0 + [A, B_, LS] + h1 and s.generated_bars == 1 and not s.done
    assert s.seg == [0] * (len(PRIMER) + 1) + g0 + [1, 1, 0] + g1
    s = stream([[A, B_], [], None])
    assert s.generated == PRIMER + [LS] + h0 + [A, B_, LS] + h1 + [LS] + h2 and s.generated_bars == 2 and not s.done
    assert s.seg == [0] * (len(PRIMER) + 1) + g0 + [1, 1, 0] + g1 + [0] + g2


def test_a_kept_empty_bar_is_not_a_drawn_bar():
    h0, _ = head(0)
    h1, _ = head(1)
    h2, _ = head(2)
    kept, drawn = stream([None, [], None]), stream([None, None, None])
    offer(kept, [LS])
    offer(drawn, [LS])
    assert drawn.generated == PRIMER + [LS] + h0 + [LS] + h1 and drawn.generated_bars == 1
    assert kept.generated == PRIMER + [LS] + h0 + [LS] + h1 + [LS] + h2 and kept.generated_bars == 2
    assert stream([None, None, None]).generated == stream(None).generated


def test_max_events_fires_inside_a_kept_bar_and_stops_the_chain():
    h0, _ = head(0)
    h1, _ = head(1)
    base = len(PRIMER) + 1 + len(h0) + 1 + len(h1)          # the length behind the Track_LeadSheet that opens bar 1
    s = stream([None, [A, B_, C, A], [C]], max_events=base + 1)
    offer(s, [LS], max_events=base + 1)
    assert s.done and s.generated == PRIMER + [LS] + h0 + [LS] + h1 + [A, B_]            # len > max_events after the second kept token
    assert s.generated_bars == 1 and s.result() == s.generated[:-1]
    # at load too
    s = stream([[A, B_, C]], max_events=len(PRIMER) + 1 + len(h0))
    assert s.done and s.generated == PRIMER + [LS] + h0 + [A]


def test_all_bars_kept_is_done_before_the_first_step_and_max_bars_cuts_the_kept_bars_too():
    h0, _ = head(0)
    h1, _ = head(1)
    h2, _ = head(2)
    s = stream([[A], [], [B_]])
    assert s.done and s.generated == PRIMER + [LS] + h0 + [A, LS] + h1 + [LS] + h2 + [B_, EOS] and s.generated_bars == 2
    s = stream([[A], [C], [B_]], max_bars=2)
    assert s.done and s.generated == PRIMER + [LS] + h0 + [A, LS] + h1 + [C, EOS]


def test_kept_tokens_pass_no_beat_check_and_the_rejection_count_restarts_behind_them():
    s = stream([None, [BEAT(9), BEAT(2)], None])
    assert offer(s, [BEAT(8), BEAT(3), LS]) == [True, False, True]           # one rejected Beat is on the count when the bar closes
    assert s.failed_cnt == 0 and s.cur_pos == 0 and s.generated_bars == 2
    assert s.generated[-len(LEAD[2]) - 4:-len(LEAD[2]) - 1] == [BEAT(9), BEAT(2), LS]
    # without a kept bar the count is carried into the next bar, as ever
    s = stream(None)
    offer(s, [BEAT(8), BEAT(3), LS])
    assert s.failed_cnt == 1 and s.cur_pos == 0


class _StreamBefore:
    """inference._Stream as it was before keep= (init and the Track_LeadSheet branch written out; the rest is the class's own offer)."""

    def __init__(self, lead, primer, max_bars):
        self.lead = lead
        self.generated = list(primer) + [LS] + list(lead[0]) + [TF]
        self.seg = [0] * len(self.generated)
        self.seg[-1] = 1
        self.target_bars = len(lead) if max_bars is None else min(max_bars, len(lead))
        self.generated_bars, self.cur_pos, self.failed_cnt = 0, 0, 0
        self.done, self.stuck = self.target_bars <= 0, False

    def offer(self, word, skip_check, max_events):
        from emo_disentanger_amd.sampling import beat_position
        ev = I2E[word]
        if not skip_check and 'Beat' in ev:
            pos = beat_position(ev)
            if not pos >= self.cur_pos:
                self.failed_cnt += 1
                if self.failed_cnt >= 256:
                    self.done = self.stuck = True
                    return True
                return False
            self.cur_pos, self.failed_cnt = pos, 0
        if ev == 'Track_LeadSheet':
            self.generated.append(word)
            self.seg.append(0)
            self.generated_bars += 1
            if self.generated_bars < self.target_bars:
                nxt = self.lead[self.generated_bars]
                self.generated.extend(nxt)
                self.seg.extend([0] * len(nxt))
                self.generated.append(TF)
                self.seg.append(1)
                self.cur_pos = 0
            else:
                self.done = True
            return True
        if ev == 'PAD_None' or (ev == 'EOS_None' and self.generated_bars < self.target_bars - 1):
            return False
        if ev == 'EOS_None' and self.generated_bars == self.target_bars - 1:
            self.generated.append(word)
            self.done = True
            return True
        self.generated.append(word)
        self.seg.append(1)
        if len(self.generated) > max_events:
            self.done = True
        return True


@pytest.mark.parametrize('run', range(len(GEN['runs'])))
def test_keep_none_gives_the_recorded_runs_of_the_reference_and_the_stream_as_it_was(run):
    from emo_disentanger_amd import inference as inf
    r = GEN['runs'][run]
    for max_bars, max_events in ((None, 200), (2, 200), (None, 40)):
        new, old = inf._Stream(E2I, LEAD, PRIMER, max_bars, keep=None), _StreamBefore(LEAD, PRIMER, max_bars)
        for w in r['sampled']:
            if new.done:
                break
            assert new.offer(w, E2I, I2E, r['skip_check'], max_events) == old.offer(w, r['skip_check'], max_events)
            assert (new.generated, new.seg, new.generated_bars, new.cur_pos, new.failed_cnt, new.done, new.stuck) == \
                (old.generated, old.seg, old.generated_bars, old.cur_pos, old.failed_cnt, old.done, old.stuck)
        if (max_bars, max_events) == (None, 200):
            assert new.done and new.result() == r['generated']


def test_bars_of_round_trips_and_refuses_what_does_not_parse():
    from emo_disentanger_amd import inference as inf
    s = stream(None)
    offer(s, [BEAT(1), A, LS, LS, B_, BEAT(3), C, LS])
    assert s.done
    piece = s.result()
    primer, lead, acc = inf.bars_of(piece, E2I)
    assert (primer, lead, acc) == (PRIMER, LEAD, [[BEAT(1), A], [], [B_, BEAT(3), C]])
    back = inf._Stream(E2I, lead, primer, None, acc, 1000)
    assert back.done and back.result() == piece
    # a piece that ended with EOS, and one cut by max_bars
    s = stream(None)
    offer(s, [A, LS, LS, C, EOS])
    assert s.done and inf._Stream(E2I, *reversed(inf.bars_of(s.result(), E2I)[:2]), None, inf.bars_of(s.result(), E2I)[2], 1000).result() == s.result()
    for bad in (PRIMER, PRIMER + [LS] + LEAD[0], PRIMER + [LS] + LEAD[0] + [TF, A, TF], PRIMER + [LS] + LEAD[0] + [TF, EOS, A],
                PRIMER + [LS] + LEAD[0] + [TF, PAD]):
        with pytest.raises(ValueError, match='bars_of'):
            inf.bars_of(bad, E2I)


def test_every_refusal_of_keep_raises():
    from emo_disentanger_amd import inference as inf
    V = len(E2I)
    ok = inf.check_keep('t', [[None, [A, B_]], None], [LEAD, LEAD], V, E2I)
    assert ok == [[None, [A, B_]], None]
    assert inf.check_keep('t', None, [LEAD], V, E2I) is None and inf.check_keep('t', [None], [LEAD], V, E2I) is None
    assert inf.check_keep('t', [[None, None]], [LEAD], V, E2I) is None           # nothing kept: the call without keep
    assert inf.check_keep('t', [[None, []]], [LEAD], V, E2I) == [[None, []]]      # an empty bar is kept
    for keep, what in (([[None]], 'keep has 1 entries for 2 inputs'), ([[None] * 4, None], 'has 4 bars, its lead sheet 3'),
                       ([[[V]], None], 'outside'), ([[[-1]], None], 'outside'), ([[[A, LS]], None], 'Track_LeadSheet'),
                       ([None, [[TF]]], 'Track_Full'), ([[[EOS]], None], 'EOS_None'), ([[[PAD]], None], 'PAD_None'), ([[7], None], 'neither None nor')):
        with pytest.raises(ValueError, match=what):
            inf.check_keep('t', keep, [LEAD, LEAD], V, E2I)
    with pytest.raises(ValueError, match='--reroll'):
        inf.parse_reroll('2:2', 3)
    with pytest.raises(ValueError, match='--reroll'):
        inf.parse_reroll('1:5', 3)
    with pytest.raises(ValueError, match='--reroll'):
        inf.parse_reroll('1-2', 3)
    assert inf.parse_reroll('0:1,2:4', 5) == [0, 2, 3]


class _Model:
    n_token = len(E2I)
    kind = 'gpt2'


def test_generate_accompaniments_refuses_before_anything_is_allocated():
    # (no GPU: every one of these is raised before the model is touched)
    from emo_disentanger_amd import inference as inf
    m = _Model()
    for kw, what in ((dict(keep=[None, None]), 'keep has 2 entries for 1 inputs'), (dict(keep=[[None] * 4]), 'has 4 bars'),
                     (dict(keep=[[[len(E2I)]]]), 'outside'), (dict(keep=[[[LS]]]), 'Track_LeadSheet'), (dict(keep=[[[TF]]]), 'Track_Full'),
                     (dict(keep=[[[EOS]]]), 'EOS_None'), (dict(keep=[[[PAD]]]), 'PAD_None')):
        with pytest.raises(ValueError, match=what):
            inf.generate_accompaniments(m, E2I, I2E, [LEAD], [PRIMER], **kw)
        with pytest.raises(ValueError, match=what):
            inf.generate_conditional_batch(m, E2I, I2E, [LEAD], [PRIMER], **kw)
    with pytest.raises(ValueError, match="window='device'.*does not read the kept-bar tables"):
        inf.generate_accompaniments(m, E2I, I2E, [LEAD], [PRIMER], keep=[[[A]]], window='device')


def test_the_packed_tables_match_their_definition():
    from emo_disentanger_amd import inference as inf
    leads = [LEAD, LEAD[:2], LEAD]
    keep = [[None, [A, B_], []], None, [[C]]]
    toks, offs, bar0, nbars, _ = inf.pack_lead_sheets(leads)
    kt, kb, ke = inf.pack_keep(keep, leads)
    assert kt.dtype == np.int64 and kb.dtype == np.int32 and ke.dtype == np.int32 and len(kb) == len(ke) == len(offs)
    for i, lead in enumerate(leads):
        for j in range(nbars[i]):
            bar = keep[i][j] if keep[i] is not None and j < len(keep[i]) else None
            t = bar0[i] + j
            assert toks[offs[t]:offs[t + 1]].tolist() == lead[j]
            if bar is None:
                assert kb[t] < 0
            else:
                assert kb[t] >= 0 and kt[kb[t]:ke[t]].tolist() == bar
        assert kb[bar0[i] + nbars[i]] < 0                      # the entry behind a stream's last bar, as lead_off has one
    assert kt.tolist() == [A, B_, C]
    # nothing kept at all: tables that mark every bar drawn, and a one-entry token table
    kt, kb, ke = inf.pack_keep([None, None, None], leads)
    assert (kb < 0).all() and len(kt) == 1
