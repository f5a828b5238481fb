"""The float64 sampler reference of the GPU sampling tests (tests/nucleus_ref.py) against the oracle's restatement of the reference's
temperature() + nucleus() (oracle/host_ref.py, itself pinned to the imported reference by tests/golden/sampling.json), on the golden fixtures and
on the random families the GPU tests use.  It also ASSERTS the two caps under which the GPU tests may exclude anything: per family at most 1/5 of
the rows are knife-edge (draw not checked) and at most 1/20 of the candidates sit on a CDF interval too narrow to probe."""
import json
import os

import numpy as np
import pytest

import nucleus_ref as nr
from oracle import host_ref

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SAMP = json.load(open(os.path.join(G, 'sampling.json')))
ROWS = 256


def _agrees_with_host(row, what):
    """host_ref's candidates of the same row lie inside the bracket and are the helper's, up to the members of a tie group at the cut."""
    try:
        cand, _ = host_ref.nucleus_candidates(host_ref.temperature(row.logits, row.temp), row.top_p)
    except IndexError:                                              # only the last sorted token crosses top_p: the helper keeps all V
        assert min(row.n_lo, row.n_hi) <= row.V <= max(row.n_lo, row.n_hi), (what, 'single crossing', row.n_lo, row.n_hi)
        return
    cand = np.asarray(cand, dtype=np.int64)
    assert min(row.n_lo, row.n_hi) <= len(cand) <= max(row.n_lo, row.n_hi), (what, len(cand), row.n_lo, row.n_hi)
    assert len(set(cand.tolist())) == len(cand)
    if row.knife:
        return
    mine = row.order[:row.n_hi]
    # the multiset of candidate probabilities (the host's fp32 sort may swap two float64 values that collide in fp32: TIE_REL)
    np.testing.assert_allclose(np.sort(row.probs[cand]), np.sort(row.probs[mine]), rtol=nr.TIE_REL, atol=0, err_msg=str(what))
    p_cut = row.ps[row.n_hi - 1]
    for t in set(cand.tolist()) ^ set(mine.tolist()):
        assert nr.same_rank(row.probs[t], p_cut), (what, 'differs by a token that is not tied with the cut', t)


@pytest.mark.parametrize('key', sorted(SAMP))
def test_golden_fixture(key):
    e = SAMP[key]
    row = nr.Row(np.array(e['logits'], dtype=np.float32), e['temp'], e['p'])
    if e['error'] == 'IndexError':
        assert key == 'flat_t1.1_p0.99' and row.n_lo == row.n_hi == row.V == 40          # the single-crossing branch
        return
    _agrees_with_host(row, key)
    cand, pr = host_ref.nucleus_candidates(host_ref.temperature(row.logits, row.temp), row.top_p)
    if not row.knife:
        # the recorded draws of the imported reference are candidates of the helper too, up to exact ties with the cut token
        mine = set(row.order[:row.n_hi].tolist())
        for t in e['observed_candidates']:
            assert t in mine or row.probs[t] == row.ps[row.n_hi - 1], (key, t)
        # and the helper's draw is the host's wherever the orders agree
        if list(cand) == list(row.cands):
            cdf = np.cumsum(pr)
            for u in (0.0, 0.25, 0.5, 0.999):
                assert nr.expected_pick(row.cands, row.probs, u) == int(cand[min(int(np.searchsorted(cdf / cdf[-1], u, side='right')), len(cand) - 1)])


def test_fixed_branches():
    rng = np.random.default_rng(5)
    for V in (1, 2, 3, 9, 327):                                     # no crossing: the top min(V, 3)
        ps = np.sort(nr.probs64(nr.family_rows(rng, V, 4.0, 1)[0], 1.2))[::-1]
        assert nr.cut_bracket(ps, 1.5, V) == (min(V, 3), min(V, 3))
    assert nr.cut_bracket(np.array([0.5, 0.5]), 0.9, 2) == (2, 2)   # single crossing: all V
    assert nr.cut_bracket(np.full(40, 0.025), 0.99, 40) == (40, 40)
    assert nr.cut_bracket(np.array([0.6, 0.3, 0.06, 0.04]), 0.5, 4) == (1, 1)      # the first crossing is kept ...
    assert nr.cut_bracket(np.array([0.6, 0.3, 0.06, 0.04]), 0.7, 4) == (2, 2)      # ... and nothing after it
    assert nr.cut_bracket(np.array([0.6, 0.3, 0.06, 0.04]), 0.95, 4) == (3, 3)
    assert nr.cut_bracket(np.array([0.6, 0.3, 0.06, 0.04]), 0.97, 4) == (4, 4)     # only the last one crosses
    # a cumulative sum within the margin of top_p is a knife edge, one a little further is not
    assert nr.cut_bracket(np.array([0.5, 0.25, 0.125, 0.125]), 0.75, 4) == (2, 3)
    assert nr.cut_bracket(np.array([0.5, 0.25, 0.125, 0.125]), 0.75 + 2 * nr.margin(4), 4) == (3, 3)


def test_order_probs_and_pick():
    p = nr.probs64(np.array([0.0, -np.inf, 2.0, 2.0, -np.inf, 0.0], dtype=np.float32), 1.2)
    assert p[1] == 0.0 and p[4] == 0.0 and abs(p.sum() - 1) < 1e-15 and p[2] == p[3] and p[0] == p[5]
    assert nr.order(p).tolist() == [2, 3, 0, 5, 1, 4]               # descending, ties by ascending index
    big = nr.probs64(np.array([233.77, 300.0, 10.0], dtype=np.float32), 1.1)        # no overflow: the maximum is subtracted
    assert np.isfinite(big).all() and big[1] > 0.999999
    cands = np.array([2, 3, 0])
    w = p[cands] / p[cands].sum()
    assert nr.expected_pick(cands, p, 0.0) == 2 and nr.expected_pick(cands, p, float(nr.U_MAX)) == 0
    assert nr.expected_pick(cands, p, w[0] - 1e-9) == 2 and nr.expected_pick(cands, p, w[0]) == 3      # side='right'
    assert nr.expected_pick(cands, p, 1.0) == 0                     # clamped
    row = nr.Row(np.array([0.0, -np.inf, 2.0, 2.0, -np.inf, 0.0], dtype=np.float32), 1.2, 1.5)
    assert (row.n_lo, row.n_hi, row.nnz, row.k_hi) == (3, 3, 4, 3)
    assert row.rank_span(2) == (0, 1) and row.rank_span(3) == (0, 1) and row.rank_span(5) == (2, 3) and row.rank_span(1) is None


def test_families_agree_with_host_and_caps_hold():
    rng = np.random.default_rng(11)
    report = []
    for V, scale, temp, top_p in nr.FAMILIES:                       # drawn family after family, in the order listed
        knife = narrow = cands = 0
        for r, logits in enumerate(nr.family_rows(rng, V, scale, ROWS)):
            row = nr.Row(logits, temp, top_p)
            _agrees_with_host(row, (V, scale, temp, top_p, r))
            if row.knife:
                knife += 1
            else:
                narrow += row.narrow()
                cands += len(row.cands)
        report.append((V, scale, temp, top_p, knife, narrow, cands))
    print('\n'.join('V %4d scale %.1f temp %.1f top_p %.2f: knife-edge %3d / %d rows, narrow intervals %d / %d candidates' % (t[:5] + (ROWS,) + t[5:])
                    for t in report))
    for V, scale, temp, top_p, knife, narrow, cands in report:
        assert 5 * knife <= ROWS, ('more than 1/5 of the rows are knife-edge', V, scale, temp, top_p, knife)
        assert cands > 0 and 20 * narrow <= cands, ('more than 1/20 of the candidates cannot be probed', V, scale, temp, top_p, narrow, cands)
