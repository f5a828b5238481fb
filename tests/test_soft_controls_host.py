"""Host (no GPU): the soft sampling controls — sampling.soft_cut_count / draw_at against a brute-force float64 version on hand-made
distributions, the draw_controls plumbing (bias rows deduplicated into the shared table, repeat, a follower inherits its leader's row,
validation before anything is allocated), event_bias / pitch_range_bias on a toy vocabulary, and the command-line flags."""
import numpy as np
import pytest

from emo_disentanger_amd import gen_loop, sampling

V = 8


def brute(probs, top_p, u, top_k=0, min_p=0.0):
    """The rule of the issue, spelled out with Python loops in float64: rank (probability descending, ties by ascending index), top-p's
    count with its three branches, min(last, k, n_m), renormalise, searchsorted(right)."""
    p = [float(x) for x in probs]
    order = sorted(range(len(p)), key=lambda i: (-p[i], i))
    sp = [p[i] for i in order]
    cum, run = [], 0.0
    for x in sp:
        run += x
        cum.append(run)
    crossings = [i for i, c in enumerate(cum) if c > top_p]
    last = min(len(p), 3) if not crossings else len(p) if len(crossings) == 1 else crossings[1]
    if top_k > 0:
        last = min(last, top_k)
    if min_p > 0:
        last = min(last, max(1, sum(1 for x in sp if x >= min_p * sp[0])))
    target = u * cum[last - 1]
    pick = sum(1 for c in cum[:last] if c <= target)
    return order[min(pick, last - 1)], last


def logits_of(probs):
    return np.log(np.array(probs, np.float64)).astype(np.float32)


# (cum of DIST: .3 .5 .7 .8 .85 .9 .95 1; of TIES: .2 .4 .6 .7 .8 .9 .95 1: top_p = 0.88 crosses at ranks 5 and 6, far from both prefixes)
DIST = [0.05, 0.3, 0.2, 0.2, 0.1, 0.05, 0.05, 0.05]
TIES = [0.1, 0.2, 0.2, 0.2, 0.1, 0.1, 0.05, 0.05]                 # a tie group (ids 1, 2, 3) on top
CASES = [
    (TIES, 0.88, 2, 0.0), (TIES, 0.88, 1, 0.0),                      # a tie group straddling k; k = 1
    (DIST, 0.88, V, 0.0), (DIST, 0.88, V + 3, 0.0), (DIST, 0.88, 0, 0.0), (DIST, 0.88, -1, -0.5),       # k = V, k > V, off
    (DIST, 0.88, 0, 1.0), (DIST, 0.88, 0, 1.7), (DIST, 0.88, 0, 0.5), (DIST, 0.88, 5, 0.3),              # min_p of 1, above 1, between
    (DIST, 1.5, 0, 0.0), (DIST, 1.5, 2, 0.0), (DIST, 1.5, 0, 0.8),                                     # no crossing (top 3), with k = 2
    ([0.125] * 8, 0.9, 0, 0.0), ([0.125] * 8, 0.9, 3, 0.0),                                            # a single crossing: all, cut by k
]


@pytest.mark.parametrize('probs, top_p, k, m', CASES)
def test_the_restatement_equals_the_brute_force_rule(probs, top_p, k, m):
    if probs[0] == 0.125:
        top_p = 0.9                                                # cum[6] = 0.875 <= 0.9 < cum[7] = 1: one crossing
    sp = np.sort(np.array(probs, np.float64))[::-1]
    for u in (0.0, 0.11, 0.37, 0.53, 0.79, 0.999):
        want, last = brute(probs, top_p, u, k, m)
        cum = np.cumsum(sp)
        i1 = int((cum <= top_p).sum())
        plain = min(V, 3) if i1 >= V else V if i1 + 1 >= V else i1 + 1
        assert sampling.soft_cut_count(sp, plain, k, m) == last
        # (float32 logits of these probabilities: the decisions above are far from rounding)
        assert sampling.draw_at(logits_of(probs), 1.0, top_p, u, top_k=k, min_p=m) == want, (u, want)


def test_named_edges():
    assert brute(TIES, 0.88, 0.999, 2)[0] == 2 and brute(TIES, 0.88, 0.0, 2)[0] == 1       # the tie group keeps its lowest indices
    assert {sampling.draw_at(logits_of(TIES), 1.0, 0.88, u, top_k=2) for u in np.linspace(0, 0.999, 50)} == {1, 2}
    assert {sampling.draw_at(logits_of(TIES), 1.0, 0.88, u, top_k=1) for u in np.linspace(0, 0.999, 50)} == {1}
    assert {sampling.draw_at(logits_of(DIST), 1.0, 0.88, u, min_p=3.0) for u in np.linspace(0, 0.999, 50)} == {1}
    assert {sampling.draw_at(logits_of(DIST), 1.0, 1.5, u, top_k=2) for u in np.linspace(0, 0.999, 50)} == {1, 2}
    sp32 = np.sort(np.array(DIST, np.float32))[::-1]
    assert sampling.soft_cut_count(sp32, 6, 0, 0.0) == 6 and sampling.soft_cut_count(sp32, 6, 4, 0.5) == 3
    # the bias is one float32 add, -inf a ban
    b = np.zeros(V, np.float32)
    b[1] = -np.inf
    assert 1 not in {sampling.draw_at(logits_of(DIST), 1.0, 0.88, u, bias=b) for u in np.linspace(0, 0.999, 50)}
    l = np.float32([0.1, 0.2])
    assert np.array_equal(sampling.biased(l, np.float32([1e-9, 3.0])), l + np.float32([1e-9, 3.0])) and sampling.biased(l, None) is l


def test_the_host_sampler_applies_the_cut():
    rng = np.random.RandomState(0)
    got = {int(sampling.nucleus(np.array(DIST, np.float32), 0.88, rng=rng, top_k=2)) for _ in range(200)}
    assert got <= {1, 2, 3} and len(got) == 2                      # (among exact ties the host order is argsort's, as for top-p)
    got = {int(sampling.nucleus(np.array(DIST, np.float32), 0.88, rng=rng, min_p=0.9)) for _ in range(50)}
    assert got == {1}
    ids, w = sampling.nucleus_candidates(np.array(DIST, np.float32), 0.55)
    assert len(ids) == 3 and abs(w.sum() - 1) < 1e-12              # without a cut: the reference's candidates


# ------------------------------------------------------------------------------------------------ draw_controls
E2I = {'Bar_None': 0, 'Note_Pitch_40': 1, 'Note_Pitch_60': 2, 'Note_Pitch_80': 3, 'Beat_0': 4, 'Chord_I_M': 5, 'EOS_None': 6, 'PAD_None': 7}


def test_bias_rows_are_deduplicated_repeated_and_inherited():
    one = {'Bar_None': 4.0}
    ctl = gen_loop.draw_controls('t', 4, V, bias=[one, None, {0: 4.0}, {5: -np.inf, 'Beat_0': 1.5}], top_k=[3, None, 0, 7], min_p=0.1, event2idx=E2I)
    t = ctl.tables()
    assert t['tok_bias'].shape == (2, V) and t['tok_bias'].dtype == np.float32 and t['bias_of'].tolist() == [0, -1, 0, 1]
    assert t['tok_bias'][0].tolist() == [4.0] + [0.0] * 7 and t['tok_bias'][1, 5] == -np.inf and t['tok_bias'][1, 4] == 1.5
    assert t['top_k_of'].tolist() == [3, 0, 0, 7] and t['top_k_of'].dtype == np.int32
    assert np.allclose(t['min_p_of'], 0.1) and t['min_p_of'].dtype == np.float32
    rep = ctl.repeat(2)
    assert rep.tables()['bias_of'].tolist() == [0, 0, -1, -1, 0, 0, 1, 1] and rep.tables()['top_k_of'].tolist() == [3, 3, 0, 0, 0, 0, 7, 7]
    # a follower gets its leader's row, cut and floor
    g = ctl.with_guidance([0.0, 0.0, 0.0, 2.0])
    assert g.n == 5 and g.tables()['bias_of'].tolist() == [0, -1, 0, 1, 1] and g.top_k_at(4) == 7 and g.min_p_at(4) == 0.1
    assert g.soft_key(4) == g.soft_key(3)
    # the form the loop classes take is read back to the same controls
    again = gen_loop.draw_controls('t', 5, V, guidance=g.guide_arg, event2idx=E2I, **g.soft_arg)
    assert again.tables()['bias_of'].tolist() == [0, -1, 0, 1, 1]
    # one value for all; a full-length array; nothing given
    allv = gen_loop.draw_controls('t', 3, V, bias=np.arange(V, dtype=np.float32), top_k=5)
    assert allv.tables()['bias_of'].tolist() == [0, 0, 0] and allv.tables()['top_k_of'].tolist() == [5, 5, 5] and 'min_p_of' not in allv.tables()
    none = gen_loop.draw_controls('t', 3, V)
    assert none.tables() == {} and none.soft_arg is None and none.bias_at(1) is None and none.top_k_at(1) == 0 and none.min_p_at(1) == 0.0
    # a pair that differs in a soft control is refused
    with pytest.raises(ValueError, match='differ in bias, top_k or min_p'):
        gen_loop.draw_controls('t', 2, V, guidance=([0, 0], [1, 1], [1.0, 1.0]), top_k=[3, 4])


@pytest.mark.parametrize('kw, what', [
    (dict(bias=[{0: 1.0}]), 'bias has 1 entries for 2 inputs'),
    (dict(bias={V: 1.0}), 'outside'), (dict(bias={-1: 1.0}), 'outside'),
    (dict(bias={'Bar_Nine': 1.0}), 'no event of the vocabulary'),
    (dict(bias={0: float('nan')}), 'NaN or \\+inf'), (dict(bias={0: float('inf')}), 'NaN or \\+inf'),
    (dict(bias=[np.zeros(V - 1), None]), 'shape'),
    (dict(top_k=2.5), 'integer'), (dict(top_k=[1, 2, 3]), '3 entries for 2 inputs'), (dict(top_k='x'), 'top_k'),
    (dict(min_p=float('nan')), 'NaN'), (dict(min_p=[0.1]), '1 entries for 2 inputs'),
])
def test_validation(kw, what):
    with pytest.raises(ValueError, match=what):
        gen_loop.draw_controls('t', 2, V, event2idx=E2I, **kw)


def test_minus_inf_is_allowed_and_an_all_zero_bias_is_none():
    ctl = gen_loop.draw_controls('t', 2, V, bias=[{0: -np.inf}, {1: 0.0}])
    assert ctl.tables()['bias_of'].tolist() == [0, -1]
    with pytest.raises(ValueError, match='bans every token'):
        gen_loop.draw_controls('t', 1, V, bias=np.full(V, -np.inf))


def test_event_bias_and_pitch_range_bias():
    from emo_disentanger_amd import inference as inf
    assert inf.event_bias(E2I, {'Bar_None': 4.0}) == {0: 4.0}
    assert inf.event_bias(E2I, {'Note_Pitch_': -2.0, 'Note_Pitch_60': 1.0}) == {1: -2.0, 2: 1.0, 3: -2.0}
    with pytest.raises(ValueError, match='neither'):
        inf.event_bias(E2I, {'Drum_': 1.0})
    assert inf.pitch_range_bias(E2I, 50, 70, -8.0) == {1: -8.0, 3: -8.0}
    assert inf.pitch_range_bias(E2I, 0, 127, -8.0) == {}
    with pytest.raises(ValueError):
        inf.pitch_range_bias({'Bar_None': 0}, 50, 70, -1.0)
    ctl = gen_loop.draw_controls('t', 1, V, bias=inf.pitch_range_bias(E2I, 50, 70, -np.inf))
    assert np.isinf(ctl.bias_at(0)[[1, 3]]).all() and ctl.bias_at(0)[2] == 0


def test_command_line_flags():
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    base2 = ['-m', 'gpt2', '-c', 'c.yaml', '-r', 'functional', '-i', 'w.pt', '-o', 'out']
    a = inf.parse_args(base2 + ['--top-k', '12', '--min-p', '0.05'])
    assert a.top_k == 12 and a.min_p == 0.05
    a = inf.parse_args(base2)
    assert a.top_k is None and a.min_p is None
    with pytest.raises(SystemExit):
        inf.parse_args(base2 + ['--top-k', '1.5'])
    with pytest.raises(SystemExit):
        inf.parse_args(base2 + ['--min-p', 'nan'])
    base1 = ['-c', 'c.yaml', '-r', 'functional', '-m', 'lead_sheet', '-i', 'w.pt', '-o', 'out']
    b = s1.parse_args(base1 + ['--top-k', '3', '--min-p', '0.2'])
    assert b.top_k == 3 and b.min_p == 0.2
    with pytest.raises(SystemExit):
        s1.parse_args(base1 + ['--min-p', 'nan'])
