"""CPU: the host-built tables behind the device grammar step of stage-1 generation (emo_txl_grammar_step) agree, token by token, with the
predicates of the reference loop (beat_position, match_emotion_key, the substring tests of generate_plain_xl), and their layout constants
with include/emo_hip.h."""
import json
import os
import pickle
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
EMOTIONS = ('Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative', 'None')


def _fixture_vocab():
    events = json.load(open(os.path.join(G, 'txl_generate.json')))['events']
    return dict(enumerate(events))


def _check_tables(i2e):
    from emo_disentanger_amd import stage1_inference as s1
    V = max(i2e) + 1
    flags, beat = s1.event_tables(i2e, V)
    assert flags.dtype == np.int32 and beat.dtype == np.int32 and flags.shape == beat.shape == (V,)
    for i, e in i2e.items():
        f = int(flags[i])
        assert bool(f & s1.EV_BEAT) == ('Beat' in e), e
        assert bool(f & s1.EV_BAR) == ('Bar' in e), e
        assert bool(f & s1.EV_PAD) == (e == 'PAD_None'), e
        assert bool(f & s1.EV_EOS) == (e == 'EOS_None'), e
        assert bool(f & s1.EV_KEY) == (e.split('_')[0] == 'Key'), e
        if 'Beat' in e:
            assert int(beat[i]) == s1.beat_position(e) == int(e.split('_')[-1])
        if f & s1.EV_KEY:
            tonic = e.partition('_')[2]
            for emo in EMOTIONS:
                mode = s1.emotion_mode({0: 'Emotion_' + emo}, 0)
                got = (mode == 1 and (f & s1.EV_MAJOR)) or (mode == 2 and (f & s1.EV_MINOR))
                assert bool(got) == bool(s1.match_emotion_key(emo, tonic)), (e, emo)
        else:
            assert not f & (s1.EV_MAJOR | s1.EV_MINOR)
    return flags, beat


def test_event_tables_agree_with_the_reference_predicates_on_the_fixture_vocabulary():
    flags, _ = _check_tables(_fixture_vocab())
    assert (flags != 0).sum() == 4 + 1 + 8 + 2            # keys, bar, beats, EOS + PAD


def test_event_tables_on_a_stage1_shaped_vocabulary():
    names = (['Emotion_%s' % e for e in EMOTIONS[:-1]] + ['Key_%s' % k for k in ('C', 'C#', 'D#', 'F#', 'A#', 'B', 'c', 'c#', 'd#', 'f#', 'a#', 'b')]
             + ['Bar_None', 'EOS_None', 'PAD_None'] + ['Beat_%d' % i for i in range(16)] + ['Chord_I_M', 'Chord_None_None', 'Note_Degree_b3']
             + ['Tempo_110', 'Key_None', 'KeyX_C'])
    i2e = dict(enumerate(names))
    flags, beat = _check_tables(i2e)
    e2i = {e: i for i, e in i2e.items()}
    assert beat[e2i['Beat_15']] == 15 and flags[e2i['Key_None']] & 16 and not flags[e2i['Key_None']] & (32 | 64)
    assert not flags[e2i['KeyX_C']] & 16


def test_emotion_modes():
    from emo_disentanger_amd import stage1_inference as s1
    i2e = {0: 'Emotion_Q1', 1: 'Emotion_Q4', 2: 'Emotion_Positive', 3: 'Emotion_Q2', 4: 'Emotion_Q3', 5: 'Emotion_Negative', 6: 'Bar_None'}
    assert [s1.emotion_mode(i2e, i) for i in range(7)] == [1, 1, 1, 2, 2, 2, 0]


def test_layout_constants_mirror_the_header():
    from emo_disentanger_amd import ops, stage1_inference as s1
    txt = open(os.path.join(ROOT, 'include', 'emo_hip.h')).read()
    enum = dict((k, int(v)) for k, v in re.findall(r'\b(EMO_TXL_[A-Z_]+)\s*=\s*(\d+)', txt))
    for py, c in (('EV_BEAT', 'EV_BEAT'), ('EV_BAR', 'EV_BAR'), ('EV_PAD', 'EV_PAD'), ('EV_EOS', 'EV_EOS'), ('EV_KEY', 'EV_KEY'),
                  ('EV_MAJOR', 'EV_MAJOR'), ('EV_MINOR', 'EV_MINOR'), ('P_MAX_BARS', 'P_MAX_BARS'), ('P_MAX_EVENTS', 'P_MAX_EVENTS'),
                  ('P_PRIMER_LEN', 'P_PRIMER_LEN'), ('P_KEYED', 'P_KEYED'), ('P_KEY_RULE', 'P_KEY_RULE'), ('P_EMO_MODE', 'P_EMO_MODE'),
                  ('S_STATUS', 'S_STATUS'), ('S_LEN', 'S_LEN'), ('S_ACCEPTED', 'S_ACCEPTED'), ('S_BEAT', 'S_BEAT'), ('S_BARS', 'S_BARS'),
                  ('S_FAILED', 'S_FAILED'), ('S_FEED', 'S_FEED'), ('S_DRAWS', 'S_DRAWS'), ('RUNNING', 'RUNNING'), ('DONE', 'DONE'),
                  ('STUCK', 'STUCK'), ('KEY_ERROR', 'KEY_ERROR'), ('OVERFLOW', 'OVERFLOW')):
        assert getattr(s1, py) == enum['EMO_TXL_' + c], py
    assert ops.TXL_PARAM_WORDS == enum['EMO_TXL_PARAM_WORDS'] and ops.TXL_STATE_WORDS == enum['EMO_TXL_STATE_WORDS']


def test_per_stream_keywords():
    from emo_disentanger_amd import stage1_inference as s1
    kw = s1._per_stream(3, max_bars=[1, 2, 3], representation='remi', prompt_bars=None)
    assert [k['max_bars'] for k in kw] == [1, 2, 3] and all(k['representation'] == 'remi' and k['prompt_bars'] is None for k in kw)
    with pytest.raises(ValueError):
        s1._per_stream(3, max_bars=[1, 2])


def test_read_vocab_appends_pad_like_the_reference(tmp_path):
    from emo_disentanger_amd import stage1_inference as s1
    events = ['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'EOS_None']
    p = tmp_path / 'dictionary.pkl'
    pickle.dump(({e: i for i, e in enumerate(events)}, {i: e for i, e in enumerate(events)}), open(p, 'wb'))
    e2i, i2e, V = s1.read_vocab(str(p))
    assert V == 6 and e2i['PAD_None'] == 5 and i2e[5] == 'PAD_None' and i2e[1] == 'Key_C'
