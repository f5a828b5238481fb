"""The device nucleus sampler (csrc/emo_nucleus.h through ops.sample_nucleus / ops.sample_nucleus_step) against the float64 reference of
tests/nucleus_ref.py, at its edges.  Every generation test downstream takes ops.sample_nucleus as the trusted restatement of the reference's
temperature() + nucleus(); this file is what holds the sampler itself.

The kernel returns one id per (row, u), so its candidate set and CDF are read by repeating one logits vector R times and sweeping u over the R
rows in ONE launch (R <= 3 V + 2).  Per row (nucleus_ref.Row.check):
  cut length    u = the largest float32 below 1 picks a token whose rank lies in the bracket [n_lo - 1, n_hi - 1]; u = 0 picks rank 0;
  containment   no pick at any probed u has rank >= n_hi, and no token of probability 0 is ever drawn;
  draw          (rows that are not knife-edge) the float32 midpoint of every CDF interval wider than 2 DELTA gives exactly that candidate, and
                b_i - 2 DELTA / b_i + 2 DELTA give candidates i / i + 1 wherever both intervals are wider than 4 DELTA.
The bounds (margin m, DELTA, TIE_REL) are derived in nucleus_ref.py; tests/test_nucleus_ref.py asserts how few rows and intervals they exclude."""
import json
import os

import numpy as np
import pytest
import torch

import nucleus_ref as nr

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SAMP = json.load(open(os.path.join(G, 'sampling.json')))
FIXTURE_TEMP_P = ((1.1, 0.99), (1.2, 0.97), (1.1, 0.9))
EDGE_V = (1, 2, 3, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024)


def _ops():
    from emo_disentanger_amd import ops
    return ops


def _sample(logits, temp, top_p, u):
    """ids [R] of ONE logits vector at the R uniforms u (the vector repeated R times, one launch)."""
    lg = torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).cuda()[None, :].repeat(len(u), 1)
    return _ops().sample_nucleus(lg, temp, top_p, torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda()).cpu().numpy()


def _sweep(row):
    """Run the probes of a row through the kernel and check them; returns the set of ids the kernel returned."""
    u, _ = row.probes()
    return row.check(u, _sample(row.logits, row.temp, row.top_p, u))


def _edge_rows():
    """(name, Row) of every edge row that is not a random family: shared by the sweep test and the step-entry test."""
    rng = np.random.default_rng(23)
    rows = []
    for V in EDGE_V:                                                # V at the kernel's structural edges: V % 8, the 512-thread stride, the LDS limit, V < 3
        rows.append(('V%d' % V, nr.Row(nr.family_rows(rng, V, 4.0, 1)[0], 1.2, 0.9)))
    lg = nr.family_rows(rng, 327, 4.0, 4)
    rows.append(('near_greedy', nr.Row(lg[0], 0.05, 0.9)))          # most exponentials underflow to 0
    rows.append(('near_greedy_p0.97', nr.Row(lg[1], 0.05, 0.97)))
    rows.append(('temp5', nr.Row(lg[2], 5.0, 0.9)))
    masked = lg[3].copy()
    masked[rng.permutation(327)[:109]] = -np.inf                    # what temperature(inadmissibles=...) produces
    rows.append(('masked_third', nr.Row(masked, 1.2, 0.9)))
    rows.append(('masked_third_p0.99', nr.Row(masked, 1.2, 0.99)))
    return rows


@pytest.mark.parametrize('fam', range(len(nr.FAMILIES)), ids=['V%d_s%g_t%g_p%g' % f for f in nr.FAMILIES])
def test_family_cut_containment_and_draw(fam):
    V, scale, temp, top_p = nr.FAMILIES[fam]
    knife = narrow = 0
    for logits in nr.family_rows(np.random.default_rng(100 + fam), V, scale, 32):
        row = nr.Row(logits, temp, top_p)
        got = _sweep(row)
        if row.knife:
            knife += 1
        else:
            narrow += row.narrow()
            want = {int(c) for c, w in zip(row.cands, row.width) if w > 2 * nr.DELTA}
            assert all(t in got or any(nr.same_rank(row.probs[t], row.probs[g]) for g in got) for t in want)
    print('V %d scale %g temp %g top_p %g: %d knife-edge rows of 32, %d narrow intervals' % (V, scale, temp, top_p, knife, narrow))
    assert 5 * knife <= 32                                          # (the stated cap, on the rows this test draws)


@pytest.mark.parametrize('key', sorted(SAMP))
def test_golden_fixture(key):
    from oracle import host_ref
    e = SAMP[key]
    logits = np.array(e['logits'], dtype=np.float32)
    if e['error'] == 'IndexError':                                  # single crossing: the kernel keeps all V
        row = nr.Row(logits, e['temp'], e['p'], n_fixed=len(logits))
        assert (row.n_lo, row.n_hi) == nr.cut_bracket(row.ps, e['p'], row.V)
        assert _sweep(row) == set(range(40))
        return
    cand, _ = host_ref.nucleus_candidates(host_ref.temperature(logits, e['temp']), e['p'])
    row = nr.Row(logits, e['temp'], e['p'])
    assert min(row.n_lo, row.n_hi) <= len(cand) <= max(row.n_lo, row.n_hi)
    if not row.knife:                                               # the expectation is the host restatement's: the recorded candidate count
        row = nr.Row(logits, e['temp'], e['p'], n_fixed=len(cand))
    got = _sweep(row)
    if key.startswith('overflow') or key.startswith('dominant'):
        assert got == {int(np.argmax(logits))} == set(e['observed_candidates'])
    if not row.knife:
        # what the imported reference was seen to draw, the kernel can draw: up to the members of an exact tie with the cut token, among which the
        # reference's choice is an accident of NumPy's unstable sort and the kernel's is the lowest indices
        p_cut = row.ps[row.n_hi - 1]
        assert all(t in got or row.probs[t] == p_cut for t in e['observed_candidates'])
        assert got == set(row.cands.tolist())                       # (every interval of the fixtures is wide enough to probe)


@pytest.mark.parametrize('V', [1, 2, 3, 9, 327])
def test_no_crossing_keeps_top_three(V):
    rng = np.random.default_rng(40 + V)
    for temp in (1.2, 1.0):
        row = nr.Row(nr.family_rows(rng, V, 4.0, 1)[0], temp, 1.5, n_fixed=min(V, 3))
        assert _sweep(row) == set(row.order[:min(V, 3)].tolist())


def test_single_crossing_keeps_all():
    row = nr.Row(np.array([0.25, 0.25], dtype=np.float32), 1.2, 0.9, n_fixed=2)      # V = 2, equal logits: only the last token crosses
    assert _sweep(row) == {0, 1}
    u = np.array([0.5 - 2 * nr.DELTA, 0.5 + 2 * nr.DELTA], dtype=np.float32)
    assert _sample(row.logits, 1.2, 0.9, u).tolist() == [0, 1]
    row = nr.Row(np.array([0.5, 0.1, 0.3, 0.2, 0.4], dtype=np.float32), 5.0, 0.9, n_fixed=5)   # nearly flat V = 5: cum = ~.21 .42 .61 .81 1
    assert (row.n_lo, row.n_hi) == nr.cut_bracket(row.ps, 0.9, 5)
    assert _sweep(row) == {0, 1, 2, 3, 4}


def test_two_equal_dominant_logits_split_at_half():
    # the case the grammar tests rely on: two equal logits far above the rest are the whole candidate set, split at u = 1/2
    rng = np.random.default_rng(31)
    for V, (a, b) in ((327, (17, 200)), (327, (326, 0)), (1024, (511, 512)), (9, (7, 8))):
        logits = nr.family_rows(rng, V, 2.0, 1)[0]
        logits[[a, b]] = 60.0
        lo, hi = min(a, b), max(a, b)
        for temp, top_p in ((1.2, 0.9), (1.0, 0.97)):
            row = nr.Row(logits, temp, top_p, n_fixed=2)
            assert (row.n_lo, row.n_hi) == nr.cut_bracket(row.ps, top_p, V)
            assert _sweep(row) == {lo, hi}
            u = np.array([0, 0.5 - 2 * nr.DELTA, 0.5 + 2 * nr.DELTA, nr.U_MAX], dtype=np.float32)
            assert _sample(logits, temp, top_p, u).tolist() == [lo, lo, hi, hi]


@pytest.mark.parametrize('temp,top_p', FIXTURE_TEMP_P)
@pytest.mark.parametrize('name', ['steps', 'steps_reversed', 'flat'])
def test_exact_ties_keep_the_lowest_indices(name, temp, top_p):
    """THIS PROJECT's tie rule (the reference's order among exact ties is an accident of NumPy's unstable sort): of a group of equal
    probabilities that straddles the cut the kernel keeps the lowest indices, and exactly as many as the reference keeps."""
    from oracle import host_ref
    logits = {'steps': np.repeat([3.0, 1.0, 0.0, -1.0], 10), 'steps_reversed': np.repeat([3.0, 1.0, 0.0, -1.0], 10)[::-1],
              'flat': np.zeros(40)}[name].astype(np.float32)
    row = nr.Row(logits, temp, top_p)
    n_lo, n_hi = min(row.n_lo, row.n_hi), max(row.n_lo, row.n_hi)
    try:
        n_host = len(host_ref.nucleus_candidates(host_ref.temperature(logits, temp), top_p)[0])
    except IndexError:
        n_host = len(logits)                                        # flat at top_p 0.99: single crossing
    assert n_lo <= n_host <= n_hi
    # the midpoints of the intervals of both ends of the bracket (the probabilities are 1/40 or more: no interval is narrow)
    u = [0.0, nr.U_MAX]
    for n in {n_lo, n_hi}:
        w = row.ps[:n]
        cdf = np.cumsum(w) / w.sum()
        u += list(cdf - 0.5 * w / w.sum())
    got = _sample(logits, temp, top_p, np.array(u, dtype=np.float32))
    k = len(set(got.tolist()))
    assert set(got.tolist()) == set(row.order[:k].tolist()), 'not the lowest indices of the tie group'
    assert n_lo <= k <= n_hi
    if not row.knife:
        assert k == n_host == n_hi
        assert _sweep(row) == set(row.order[:k].tolist())
        exact = _sample(logits, temp, top_p, np.array(u[2:], dtype=np.float32))
        assert exact.tolist() == row.order[:k].tolist()             # and in ascending index inside every group, not merely as a set


def test_edge_rows():
    for name, row in _edge_rows():
        got = _sweep(row)
        assert all(row.probs[t] > 0 for t in got), name
        if not row.knife:
            want = {int(c) for c, w in zip(row.cands, row.width) if w > 2 * nr.DELTA}
            assert want <= got, name


def test_masked_ids_are_never_drawn():
    rng = np.random.default_rng(37)
    logits = nr.family_rows(rng, 327, 4.0, 1)[0]
    masked = rng.permutation(327)[:109]
    logits[masked] = -np.inf
    u = np.concatenate([np.linspace(0, 1, 1024, endpoint=False, dtype=np.float32), [nr.U_MAX, np.nextafter(nr.U_MAX, np.float32(0))]])
    for temp, top_p in ((1.2, 0.9), (1.2, 0.999), (5.0, 1.5)):
        got = _sample(logits, temp, top_p, u)
        assert not set(got.tolist()) & set(masked.tolist())
    # only 2 finite logits in V = 327: cum = p0, 1, 1, ... so the second crossing is reached at once and the zero-probability tail stays out
    # (a single crossing cannot coexist with such a tail: cum is flat over it, so a crossing at the last position is also one before it) ...
    two = np.full(327, -np.inf, dtype=np.float32)
    two[[300, 5]] = [1.0, 0.5]
    row = nr.Row(two, 1.2, 0.9)
    assert (row.n_lo, row.n_hi, row.nnz) == (2, 2, 2)
    assert _sweep(row) == {300, 5}
    assert set(_sample(two, 1.2, 0.9, u).tolist()) == {300, 5}
    # ... while the no-crossing branch does take its top 3 out of 2 drawable tokens, and V = 3 keeps all V with one of them masked
    row = nr.Row(two, 1.2, 1.5, n_fixed=3)
    assert row.k_hi == 2 and _sweep(row) == {300, 5}
    assert set(_sample(two, 1.2, 1.5, u).tolist()) == {300, 5}
    three = np.array([-np.inf, 0.0, 0.0], dtype=np.float32)
    assert set(_sample(three, 1.2, 0.9, u).tolist()) == {1, 2}


@pytest.mark.parametrize('rows', [1, 33])
def test_step_entry_is_bitwise_the_sampler(rows):
    """ops.sample_nucleus_step on the edge rows: ids, seq and step are those of ops.sample_nucleus on the uniforms u[step[r], r]."""
    ops = _ops()
    rng = np.random.default_rng(50 + rows)
    edge = _edge_rows()
    K, col0 = 5, 2
    for V in sorted({row.V for _, row in edge}):
        pool = [row for _, row in edge if row.V == V]
        pick = [pool[r % len(pool)] for r in range(rows)]
        temp, top_p = pick[0].temp, pick[0].top_p
        logits = np.stack([row.logits for row in pick])
        logits[1::2] = logits[1::2][:, ::-1]                        # (rows of one launch share temp and top_p; vary the vectors instead)
        U = rng.random((K, rows)).astype(np.float32)
        U[0, 0], U[K - 1, rows - 1] = 0.0, nr.U_MAX
        step0 = (np.arange(rows) * 3 + K - 1) % K
        lg, Ud, step = torch.from_numpy(logits).cuda(), torch.from_numpy(U).cuda(), torch.from_numpy(step0).cuda()
        seq = torch.full((rows, col0 + K + 1), -1, dtype=torch.long).cuda()
        u_rows = Ud[step, torch.arange(rows).cuda()].contiguous()
        ref = ops.sample_nucleus(lg, temp, top_p, u_rows)
        tok = ops.sample_nucleus_step(lg, temp, top_p, Ud, step, seq=seq, col0=col0)
        exp_seq = torch.full((rows, col0 + K + 1), -1, dtype=torch.long)
        exp_seq[torch.arange(rows), col0 + torch.from_numpy(step0)] = ref.cpu()
        assert torch.equal(tok, ref) and torch.equal(seq.cpu(), exp_seq) and torch.equal(step.cpu(), torch.from_numpy(step0) + 1), V
        for r in (0, rows - 1):                                     # and the shared reference run is itself right
            row = nr.Row(logits[r], temp, top_p)
            if not row.knife:
                t, c = int(ref[r]), nr.expected_pick(row.cands, row.probs, float(u_rows[r]))
                d = np.abs(row.cdf - float(u_rows[r])).min()
                assert t == c or nr.same_rank(row.probs[t], row.probs[c]) or d <= nr.DELTA, (V, r, t, c)


@pytest.mark.parametrize('V,temp,what', [(1025, 1.2, 'V must be <= 1024'), (327, 0.0, 'temperature must be > 0'), (327, -1.0, 'temperature must be > 0')])
def test_refusals_leave_the_output_alone(V, temp, what):
    """Argument checks on the host: an error code, the message in emo_last_error, nothing launched and the output untouched."""
    from emo_disentanger_amd._lib import EmoError, lib, ptr, stream
    ops = _ops()
    lg, u = torch.zeros(2, V, device='cuda'), torch.full((2,), 0.5, device='cuda')
    out = torch.full((2,), -7, dtype=torch.long, device='cuda')
    assert lib.emo_sample_nucleus(ptr(lg), 2, V, temp, 0.9, ptr(u), ptr(out), stream()) != 0
    assert what in lib.emo_last_error().decode() and 'emo_sample_nucleus:' in lib.emo_last_error().decode()
    U, step, seq = torch.full((3, 2), 0.5, device='cuda'), torch.tensor([1, 2], device='cuda'), torch.full((2, 6), -1, dtype=torch.long, device='cuda')
    with pytest.raises(EmoError, match=what):
        ops.sample_nucleus_step(lg, temp, 0.9, U, step, seq=seq, col0=1, out=out)
    assert 'emo_sample_nucleus_step:' in lib.emo_last_error().decode()
    with pytest.raises(EmoError, match=what):
        ops.sample_nucleus(lg, temp, 0.9, u)
    torch.cuda.synchronize()
    assert out.tolist() == [-7, -7] and step.tolist() == [1, 2] and bool((seq == -1).all())
