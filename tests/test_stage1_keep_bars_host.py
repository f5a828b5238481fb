"""CPU: the host side of kept bars in stage-1 generation: the rule (_LeadSheet with keep, against a plain restatement written here), keep=None
and an all-None list leave the token lists as they were, bars_of round-trips, every refusal of check_keep, the packed tables, the command line,
block_set's checks of the new fields and the entry's refusals for both stage-1 kinds, named by kind (nothing is launched)."""
import ctypes

import numpy as np
import pytest
import torch

NAMES = (['Emotion_Positive', 'Emotion_Negative', 'Key_C', 'Key_c', 'Bar_None', 'PAD_None', 'EOS_None'] + ['Beat_%d' % k for k in range(16)]
         + ['Note_%d' % k for k in range(10)])
E2I = {e: i for i, e in enumerate(NAMES)}
I2E = dict(enumerate(NAMES))
V = len(NAMES)
BAR, PAD, EOS = E2I['Bar_None'], E2I['PAD_None'], E2I['EOS_None']
PRIMER = ['Emotion_Positive', 'Key_C']


def N(k):
    return E2I['Note_%d' % k]


def BT(k):
    return E2I['Beat_%d' % k]


def sheet(keep, max_bars=8, max_events=100, primer=PRIMER, prompt_bars=None):
    from emo_disentanger_amd import stage1_inference as s1
    return s1._LeadSheet(E2I, primer, prompt_bars, max_bars, max_events, keep)


def offer(s, words):
    return [s.offer(w, I2E[w]) for w in words if not s.finished and s.bars < s.max_bars]


def restated(words, keep, max_bars=8, max_events=100, primer=PRIMER):
    """The rule, written out plainly: -> (tokens, bars, beat, rejected in a row, accepted, over)."""
    toks, bars, beat, rej, acc, over = [E2I[e] for e in primer], 0, 0, 0, 0, False
    for w in words:
        if over:
            break
        e = I2E[w]
        if e.startswith('Beat_'):
            if int(e[5:]) < beat:
                rej += 1
                continue
            beat, rej = int(e[5:]), 0
        if e == 'PAD_None':
            continue
        toks.append(w)
        acc += 1
        if e == 'Bar_None':
            j, bars, beat = bars, bars + 1, 0
            over = len(toks) > max_events or bars >= max_bars
            while not over and keep is not None and j < len(keep) and keep[j] is not None:
                beat = rej = 0
                for t in keep[j]:
                    toks.append(t)
                    if len(toks) > max_events:
                        over = True
                        break
                if over:
                    break
                toks.append(BAR)
                bars += 1
                over = len(toks) > max_events or bars >= max_bars
                j += 1
        else:
            over = len(toks) > max_events or e == 'EOS_None'
    return toks, bars, beat, rej, acc, over


CASES = [
    ('a kept bar after a drawn one', [None, [BT(3), N(1)]], dict(), [BAR, BT(2), N(0), BAR, BT(1), N(2), BAR]),
    ('two consecutive kept bars', [None, [N(1)], [BT(9), N(2)], None], dict(), [BAR, N(0), BAR, BT(4), N(3)]),
    ('an empty kept bar', [[], None], dict(), [BAR, BT(5), N(1)]),
    ('a kept first bar and everything behind it', [[N(1)], [N(2)], [N(3)]], dict(max_bars=4), [BAR, N(9)]),
    ('a kept last bar', [None, [N(1), N(2)]], dict(max_bars=3), [N(0), BAR, BT(7), BAR, N(5)]),
    ('max_events inside a kept bar', [[N(1), N(2), N(3), N(4)]], dict(max_events=5), [BAR, N(5)]),
    ('max_events at the closing Bar', [[N(1), N(2)]], dict(max_events=5), [BAR, N(5)]),
    ('a rejected beat on the count when the chain fires', [None, [BT(9)]], dict(), [BAR, BT(8), BT(3), BAR, BT(2), BT(1)]),
]


@pytest.mark.parametrize('what, keep, kw, words', CASES, ids=[c[0] for c in CASES])
def test_the_rule_against_its_restatement(what, keep, kw, words):
    s = sheet(keep, **kw)
    offer(s, words)
    toks, bars, beat, rej, acc, over = restated(words, keep, **kw)
    assert (s.tokens, s.bars, s.beat, s.rejected_in_a_row, s.accepted, not s.open()) == (toks, bars, beat, rej, acc, over), what


def test_the_cases_are_what_they_say():
    s = sheet([None, [BT(3), N(1)]])
    assert offer(s, [BAR, BT(2), N(0), BAR]) == [True] * 4
    assert s.tokens == [0, 2, BAR, BT(2), N(0), BAR, BT(3), N(1), BAR] and s.chained == 3 and s.bars == 3 and s.accepted == 4
    assert (s.beat, s.rejected_in_a_row) == (0, 0) and s.offer(BT(1), 'Beat_1') and s.chained == 0          # Beat 1 behind the kept Beat 3: position 0
    s = sheet([None, [N(1), N(2)]], max_bars=3)
    offer(s, [N(0), BAR, BT(7), BAR, N(5)])
    assert not s.open() and not s.finished and s.tokens[-4:] == [BAR, N(1), N(2), BAR] and s.bars == 3     # tokens[:-1] drops the forced closing Bar
    s = sheet([[N(1), N(2), N(3), N(4)]], max_events=5)
    offer(s, [BAR])
    assert s.finished and s.tokens == [0, 2, BAR, N(1), N(2), N(3)] and s.bars == 1
    s = sheet([None, [BT(9)]])
    offer(s, [BAR, BT(8), BT(3)])
    assert s.rejected_in_a_row == 1
    offer(s, [BAR])
    assert (s.beat, s.rejected_in_a_row) == (0, 0)
    s = sheet([None, None])                                                 # without a kept bar in between the count is carried, as ever
    offer(s, [BAR, BT(8), BT(3), BAR])
    assert s.rejected_in_a_row == 1 and s.chained == 0


def test_keep_none_and_an_all_none_list_leave_the_token_lists_as_they_were():
    rs = np.random.RandomState(3)
    for trial in range(20):
        words = [int(w) for w in rs.choice([BAR, BAR, PAD, BT(1), BT(5), BT(9), N(1), N(2), N(3)], size=60)]
        a, b, c = sheet(None, 5, 40), sheet([None] * 7, 5, 40), sheet([], 5, 40)
        ra, rb, rc = offer(a, words), offer(b, words), offer(c, words)
        assert ra == rb == rc and a.tokens == b.tokens == c.tokens == restated(words, None, 5, 40)[0]
        assert (a.bars, a.beat, a.rejected_in_a_row, a.accepted, a.finished) == (b.bars, b.beat, b.rejected_in_a_row, b.accepted, b.finished)
    assert not hasattr(sheet(None), 'bar_id')


def test_bars_of_round_trips_and_refuses_what_does_not_parse():
    from emo_disentanger_amd import stage1_inference as s1
    s = sheet(None, max_bars=4)
    offer(s, [N(0), BAR, BT(1), N(1), BAR, BAR, N(2), BT(3), BAR])
    ids = s.tokens[:-1]
    head, bars, ended = s1.bars_of(ids, E2I)
    assert head == [0, 2, N(0)] and bars == [[BT(1), N(1)], [], [N(2), BT(3)]] and not ended
    back = head + [t for b in bars for t in [BAR] + b]
    assert back == ids
    head2, bars2, ended2 = s1.bars_of(s.tokens, E2I)
    assert (head2, bars2, ended2) == (head, bars + [[]], True) and head2 + [t for b in bars2 for t in [BAR] + b] == s.tokens
    # fed back as a primer and an all-kept keep, the piece is reproduced from its first Bar on
    again = sheet(bars, max_bars=len(bars) + 1, primer=[I2E[t] for t in head])
    offer(again, [BAR])
    assert again.tokens[:-1] == ids and not again.open()
    for bad, what in (([0, 2, N(1)], 'no Bar_None'), ([0, BAR, N(1), EOS], 'EOS_None'), ([0, BAR, PAD], 'PAD_None')):
        with pytest.raises(ValueError, match=what):
            s1.bars_of(bad, E2I)


def test_every_refusal_of_keep_raises():
    from emo_disentanger_amd import stage1_inference as s1
    ok = s1.check_keep('t', [[None, (N(1), N(2))], None], 2, V, I2E)
    assert ok == [[None, [N(1), N(2)]], None]
    assert s1.check_keep('t', None, 2, V, I2E) is None and s1.check_keep('t', [[None], None], 2, V, I2E) is None
    for keep, kw, what in [([[None]], {}, 'keep has 1 entries for 2 primers'),
                           ([[[V]], None], {}, r'keep\[0\]\[0\] holds token id %d outside \[0, %d\)' % (V, V)),
                           ([[[-1]], None], {}, 'outside'),
                           ([None, [None, [N(1), BAR]]], {}, r'keep\[1\]\[1\] holds Bar_None'),
                           ([[[PAD]], None], {}, 'holds PAD_None'), ([[[EOS]], None], {}, 'holds EOS_None'),
                           ([[5], None], {}, 'neither None nor a sequence'),
                           ([[[N(1)], None], None], dict(prompt_bars=1), r'keep\[0\]\[0\] lies under prompt_bars = 1'),
                           ([None, [None, [N(1)]]], dict(prompt_bars=[0, 2]), r'keep\[1\]\[1\] lies under prompt_bars = 2')]:
        with pytest.raises(ValueError, match=what):
            s1.check_keep('t', keep, 2, V, I2E, **kw)
    assert s1.check_keep('t', [[None, [N(1)]], None], 2, V, I2E, prompt_bars=1) is not None


class _Model:
    vocab_size = V

    def parameters(self):
        raise AssertionError('refused before the model is touched')


def test_generate_lead_sheets_refuses_before_anything_is_allocated():
    from emo_disentanger_amd import stage1_inference as s1
    for keep, what in (([[None]] * 3, 'keep has 3 entries for 2 primers'), ([[[BAR]], None], 'holds Bar_None')):
        with pytest.raises(ValueError, match=what):
            s1.generate_lead_sheets(_Model(), E2I, I2E, [PRIMER, PRIMER], keep=keep)
        with pytest.raises(ValueError, match=what):
            s1.generate_plain_xl_batch(_Model(), E2I, I2E, [PRIMER, PRIMER], keep=keep)
    with pytest.raises(ValueError, match='lies under prompt_bars'):
        s1.generate_lead_sheets(_Model(), E2I, I2E, [PRIMER, PRIMER], keep=[[[N(1)]], None], prompt_bars=1)


def test_the_packed_tables_match_their_definition():
    from emo_disentanger_amd import stage1_inference as s1
    keep = [[None, [N(1), N(2)], []], None, [[N(3)]]]
    tok, beg, end, k0, kn = s1.pack_keep(keep)
    assert tok.tolist() == [N(1), N(2), N(3)] and beg.tolist() == [-1, 0, 2, 2] and end.tolist() == [0, 2, 2, 3]
    assert k0.tolist() == [0, 3, 3] and kn.tolist() == [3, 0, 1]
    assert (tok.dtype, beg.dtype, end.dtype, k0.dtype) == (np.int64, np.int32, np.int32, np.int32)
    for i, bars in enumerate(keep):
        for j, bar in enumerate(bars or ()):
            assert (None if beg[k0[i] + j] < 0 else tok[beg[k0[i] + j]:end[k0[i] + j]].tolist()) == bar
    _, _, _, k0, kn = s1.pack_keep(keep + [keep[0]], table_of=[0, 1, 2, 0])                 # a follower reads its leader's entries
    assert (k0[3], kn[3]) == (k0[0], kn[0])
    assert s1.longest_kept_run(keep[0]) == 4 and s1.longest_kept_run(None) == 0 and s1.longest_kept_run([[N(1)], None, [N(1), N(2)]]) == 3


def test_the_command_line_parses_and_refuses():
    from emo_disentanger_amd import stage1_inference as s1
    base = ['-c', 'c.yaml', '-r', 'functional', '-m', 'lead_sheet']
    a = s1.parse_args(base + ['--variation-of', 'x/samp_00_Positive_roman.txt', '--reroll', '4:8,10:11'])
    assert a.variation_of.endswith('roman.txt') and a.reroll == '4:8,10:11'
    for bad in (['--variation-of', 'f.txt'], ['--reroll', '1:2'], ['--variation-of', 'f.txt', '--reroll', '1:2', '--exact']):
        with pytest.raises(SystemExit):
            s1.parse_args(base + bad)
    assert s1.parse_reroll('4:8,10:11', 12) == [4, 5, 6, 7, 10]
    for spec in ('4:13', '3:3', 'x', '-1:2'):
        with pytest.raises(ValueError):
            s1.parse_reroll(spec, 12)


def test_read_variation_takes_the_emotion_from_the_name(tmp_path):
    from emo_disentanger_amd import stage1_inference as s1
    f = tmp_path / 'samp_03_Negative_roman.txt'
    f.write_text('\n'.join(['Key_c', 'Bar_None', 'Beat_1', 'Note_1', 'Bar_None', 'Note_2']) + '\n')
    assert s1.read_variation(str(f), E2I, ('Positive', 'Negative')) == ('Negative', [E2I['Key_c']], [[BT(1), N(1)], [N(2)]])
    g = tmp_path / 'piece.txt'
    g.write_text('Key_c\nBar_None\n')
    with pytest.raises(ValueError, match='emotions'):
        s1.read_variation(str(g), E2I, ('Positive', 'Negative'))
    f.write_text('Key_c\nBar_None\nNo_Such\n')
    with pytest.raises(ValueError, match='not an event'):
        s1.read_variation(str(f), E2I, ('Positive', 'Negative'))


# ------------------------------------------------------------------------------------------------ the block
NEW = ('keep_tok', 'keep_beg', 'keep_end', 'keep_left')


def test_the_mirror_holds_the_two_new_fields_behind_keep_eos():
    from emo_disentanger_amd import _lib
    G = _lib.GrammarStep
    names = [f[0] for f in G._fields_]
    at = names.index('keep_eos')
    assert names[at + 1:at + 4] == ['keep_bar', 'keep_left', 'track_full'] and dict(G._fields_)['keep_left'] is _lib.c_p
    assert G.keep_bar.offset == G.keep_eos.offset + 8 and G.keep_left.offset == G.keep_bar.offset + 8
    assert names[-3:] == ['tok_logp', 'tok_rank', 'tok_entropy'] and names[-4] == 'row_reset'
    assert ctypes.sizeof(G) == _lib.lib.emo_grammar_step_size()


def _tables(n=3):
    params = torch.zeros(n, 8, dtype=torch.int32)
    params[:, 6], params[:, 7] = torch.tensor([0, 2, 2]), torch.tensor([2, 0, 1])
    return dict(params=params, keep_tok=torch.tensor([N(1), N(2), N(3)]), keep_beg=torch.tensor([-1, 0, 2], dtype=torch.int32),
                keep_end=torch.tensor([0, 2, 3], dtype=torch.int32), keep_left=torch.zeros(n, dtype=torch.int32))


@pytest.mark.parametrize('kind, name', [(0, 'txl'), (3, 'txl_queue')])
def test_block_set_takes_a_sound_set_and_refuses_every_other(monkeypatch, kind, name):
    from emo_disentanger_amd import ops
    monkeypatch.setattr(ops, 'ptr', lambda t: None if t is None else t.data_ptr())
    num = dict(n_rows=3, ld_u=3, n_token=V, n_keep=3, keep_bar=BAR, ld_seq=32)
    args, held = ops.GrammarStep(kind=kind), {}
    ops.block_set(args, held, **num, **_tables())
    assert all(getattr(args, k) == held[k].data_ptr() for k in NEW) and args.keep_bar == BAR
    who = r'grammar step\[%s\]: ' % name
    for drop in NEW:                                                            # a partial set
        args, held = ops.GrammarStep(kind=kind), {}
        with pytest.raises(AssertionError, match=who + 'keep_tok, keep_beg, keep_end and keep_left come together or not at all'):
            ops.block_set(args, held, **num, **{k: v for k, v in _tables().items() if k != drop})
        assert all(getattr(args, k) is None for k in NEW) and not set(NEW) & set(held)      # a refused set never stays in the block
    for k, bad in (('keep_tok', torch.zeros(3, dtype=torch.int32)), ('keep_beg', torch.zeros(3, dtype=torch.int64)),
                   ('keep_end', torch.zeros(3)), ('keep_left', torch.zeros(3, dtype=torch.int64)), ('keep_left', torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(AssertionError, match='bad dtype / layout of ' + k):
            ops.block_set(ops.GrammarStep(kind=kind), {}, **num, **dict(_tables(), **{k: bad}))
    for change, what in ((dict(keep_end=torch.tensor([0, 2, 4], dtype=torch.int32)), 'a kept bar lies outside'),
                         (dict(keep_end=torch.tensor([0, -1, 3], dtype=torch.int32)), 'a kept bar lies outside'),
                         (dict(keep_end=torch.tensor([0, 2], dtype=torch.int32)), 'one length'),
                         (dict(keep_left=torch.tensor([0, 40, 0], dtype=torch.int32)), 'keep_left lies outside'),
                         (dict(keep_beg=torch.tensor([-1, 0], dtype=torch.int32), keep_end=torch.tensor([0, 2], dtype=torch.int32)), 'lies outside keep_beg')):
        with pytest.raises(AssertionError, match=who + '.*' + what):
            ops.block_set(ops.GrammarStep(kind=kind), {}, **num, **dict(_tables(), **change))
    for bar in (-1, V):
        with pytest.raises(AssertionError, match=who + r'keep_bar = %d lies outside \[0, %d\)' % (bar, V)):
            ops.block_set(ops.GrammarStep(kind=kind), {}, **dict(num, keep_bar=bar), **_tables())
    # a new params is held to the tables the block already has
    args, held = ops.GrammarStep(kind=kind), {}
    ops.block_set(args, held, **num, **_tables())
    worse = torch.zeros(3, 8, dtype=torch.int32)
    worse[2, 6], worse[2, 7] = 2, 2
    with pytest.raises(AssertionError, match=who + '.*lies outside keep_beg'):
        ops.block_set(args, held, params=worse)
    assert args.keep_tok is None and 'keep_tok' not in held
    t = _tables()
    del t['params']
    with pytest.raises(AssertionError, match=who + 'the kept-bar tables are indexed by params'):
        ops.block_set(ops.GrammarStep(kind=kind), {}, **num, **t)


def _args(kind, **kw):
    from emo_disentanger_amd import _lib
    a = _lib.GrammarStep()
    for name, ctype in _lib.GrammarStep._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.kind, a.n_rows, a.n_token, a.n_u, a.ld_u, a.ld_seq, a.n_jobs, a.mem_rows = kind, 3, 327, 8, 3, 64, 3, 16
    a.temperature, a.top_p, a.key_temperature, a.key_top_p = 1.2, 0.9, 1.1, 0.97
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('kind, name', [(0, 'txl'), (3, 'txl_queue')])
def test_both_stage1_kinds_refuse_a_partial_set_without_a_gpu_and_name_their_kind(kind, name):
    from emo_disentanger_amd import _lib
    want = 'emo_grammar_step[%s]: keep_tok, keep_beg, keep_end and keep_left come together or not at all, with 0 <= n_keep < 2^31' % name
    for kw in [{k: None} for k in NEW] + [dict(keep_tok=None, keep_left=None), dict(n_keep=-1), dict(n_keep=2 ** 31)]:
        assert _lib.lib.emo_grammar_step(ctypes.byref(_args(kind, **kw)), None) == -1
        assert _lib.lib.emo_last_error().decode() == want, kw
    for bar in (-1, 327):
        assert _lib.lib.emo_grammar_step(ctypes.byref(_args(kind, keep_bar=bar)), None) == -1
        assert _lib.lib.emo_last_error().decode() == 'emo_grammar_step[%s]: keep_bar %d lies outside [0, V)' % (name, bar)
    # the new check comes behind every other one of the kind
    assert _lib.lib.emo_grammar_step(ctypes.byref(_args(kind, keep_tok=None, temperature=0.0)), None) == -1
    assert _lib.lib.emo_last_error().decode() == 'emo_grammar_step[%s]: temperatures must be > 0' % name
    assert _lib.lib.emo_grammar_step(ctypes.byref(_args(kind, keep_left=None, guide_scale=None)), None) == -1
    assert ('guide_cond' in _lib.lib.emo_last_error().decode()) == (kind == 0)
