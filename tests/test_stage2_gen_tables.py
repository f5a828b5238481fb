"""CPU: the host-built tables behind the device grammar step of stage-2 generation (emo_acc_grammar_step) agree, token by token, with the
tests _Stream.offer makes (beat_position, Track_LeadSheet, PAD, EOS); their layout constants mirror include/emo_hip.h; the lead-sheet packing
round-trips; and generate_accompaniments refuses what the device loop does not do."""
import json
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')


def _check_tables(i2e):
    from emo_disentanger_amd import inference as inf
    V = max(i2e) + 1
    flags, beat = inf.acc_event_tables(i2e, V)
    assert flags.dtype == np.int32 and beat.dtype == np.int32 and flags.shape == beat.shape == (V,)
    for i, e in i2e.items():
        f = int(flags[i])
        assert bool(f & inf.ACC_EV_BEAT) == ('Beat' in e), e
        assert bool(f & inf.ACC_EV_TRACK_LS) == (e == 'Track_LeadSheet'), e
        assert bool(f & inf.ACC_EV_PAD) == (e == 'PAD_None'), e
        assert bool(f & inf.ACC_EV_EOS) == (e == 'EOS_None'), e
        assert int(beat[i]) == (inf.beat_position(e) if 'Beat' in e else 0), e
    return flags, beat


def test_acc_event_tables_agree_with_the_host_grammar_on_the_fixture_vocabulary():
    events = json.load(open(os.path.join(G, 'generate.json')))['events']
    flags, beat = _check_tables(dict(enumerate(events)))
    assert (flags != 0).sum() == 16 + 1 + 1 + 1                # Beat_0..15, Track_LeadSheet, EOS, PAD
    assert beat[events.index('Beat_15')] == 15


def test_acc_event_tables_on_a_full_size_vocabulary():
    from emo_disentanger_amd import inference as inf
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4')] + ['Key_%s' % k for k in ('C', 'a', 'G', 'e')] + ['Tempo_110']
             + ['Track_LeadSheet', 'Track_Full', 'Bar_None'] + ['Beat_%d' % i for i in range(16)] + ['Chord_%d_M' % i for i in range(40)])
    names += ['Note_Pitch_%d' % i for i in range(327 - 2 - len(names))] + ['EOS_None', 'PAD_None']
    assert len(names) == 327
    i2e = dict(enumerate(names))
    flags, _ = _check_tables(i2e)
    e2i = {e: i for i, e in i2e.items()}
    assert flags[e2i['Track_Full']] == 0 and flags[e2i['Bar_None']] == 0          # no Bar rule in stage 2
    # ids without an event (a vocabulary shorter than the model's output) get no bits
    f2, b2 = inf.acc_event_tables(i2e, 340)
    assert (f2[327:] == 0).all() and (b2[327:] == 0).all()


def test_layout_constants_mirror_the_header():
    from emo_disentanger_amd import inference as inf, ops
    txt = open(os.path.join(ROOT, 'include', 'emo_hip.h')).read()
    enum = dict((k, int(v)) for k, v in re.findall(r'\b(EMO_ACC_[A-Z0-9_]+)\s*=\s*(\d+)', txt))
    names = ['EV_BEAT', 'EV_TRACK_LS', 'EV_PAD', 'EV_EOS', 'P_TARGET_BARS', 'P_MAX_EVENTS', 'P_SKIP_CHECK', 'P_BAR0', 'P_N_BARS',
             'S_STATUS', 'S_LEN', 'S_CONSUMED', 'S_BARS', 'S_CUR_POS', 'S_FAILED', 'S_DRAWS', 'S_ACCEPTED',
             'RUNNING', 'DONE', 'STUCK', 'WINDOW', 'OUT_OF_DRAWS', 'OVERFLOW']
    for nm in names:
        assert getattr(inf, 'ACC_' + nm) == enum['EMO_ACC_' + nm], nm
    assert ops.ACC_PARAM_WORDS == enum['EMO_ACC_PARAM_WORDS'] and ops.ACC_STATE_WORDS == enum['EMO_ACC_STATE_WORDS']
    assert len(enum) == len(names) + 2


def test_lead_sheet_packing_round_trips():
    from emo_disentanger_amd import inference as inf
    leads = [[[9, 10, 30], [9, 14]], [[9]], [[9, 10, 30, 26, 27, 28], [9, 11], [9, 12, 13]], [[9, 1, 2, 3, 4, 5, 6, 7]]]
    toks, offs, bar0, nbars, longest = inf.pack_lead_sheets(leads)
    assert toks.dtype == np.int64 and offs.dtype == np.int32
    assert nbars == [2, 1, 3, 1] and longest == 8
    assert len(offs) == sum(nb + 1 for nb in nbars) and offs[-1] == len(toks) == sum(len(b) for ld in leads for b in ld)
    assert (np.diff(offs) >= 0).all()
    # bar j of stream i, read as the kernel reads it
    assert [[toks[offs[b0 + j]:offs[b0 + j + 1]].tolist() for j in range(nb)] for b0, nb in zip(bar0, nbars)] == leads


def test_device_loop_refuses_inadmissibles_and_large_vocabularies():
    from emo_disentanger_amd import inference as inf
    from emo_disentanger_amd._lib import EmoError
    small, big = types.SimpleNamespace(n_token=327), types.SimpleNamespace(n_token=1025)
    lead, primer = [[[9, 10]]], [[0, 4, 6]]
    with pytest.raises(ValueError):
        inf.generate_accompaniments(small, {}, {}, lead, primer, inadmissibles=[3])
    with pytest.raises(EmoError):
        inf.generate_accompaniments(big, {}, {}, lead, primer)
