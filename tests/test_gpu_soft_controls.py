"""GPU: the soft sampling controls of emo_grammar_step (tok_bias / n_biases / bias_of / top_k_of / min_p_of), kernel level, on synthetic fp32
logits and the small synthetic event tables of test_gpu_sampling_controls.py (its Rig), all five kinds driven directly:
  1. a biased launch on raw logits is bit for bit the unbiased launch on logits that NumPy float32 `l + b` wrote (for a guided pair: `l` the
     host-combined row, the leader's bias row), with and without bans and per-stream temp / top_p on top, over a script of launches (primer
     feed, rejections / in-launch redraws, accepted draws, an ending, queue admissions); -inf entries against the same entries as a ban;
     bias_of values of -1 and n_biases read as "no bias";
  2. the ids drawn under top_k / min_p are those of the float64 restatement sampling.draw_at, on rows whose margins (asserted on the inputs)
     keep every decision away from float32 rounding; the edges on the device: k = 1, exact ties across k, min_p > 1, a cut on top of top-p's
     no-crossing and single-crossing rules;
  3. the recorded scores under the controls are the model's, from the unbiased row;
  4. with every new field NULL nothing changes (the one test here that passes without the feature)."""
import numpy as np
import pytest
import torch

import nucleus_ref as nr
import test_gpu_sampling_controls as hc
from test_gpu_draw_scores import row_tol
from test_gpu_sampling_controls import ACC, ACCQ, DEV, KINDS, S_ACCEPTED, S_DRAWS, S_LEN, TABLES, TXL, TXLQ, WIN, Rig, T, pack

pytestmark = pytest.mark.gpu


def set_bias(rig, table, bias_of, raw=False):
    """The bias table into a built rig's block; raw: bias_of behind block_set's back (it refuses rows outside [-1, n_biases))."""
    ops = hc._ops()
    if raw:
        ops.block_set(rig.args, rig.held, n_biases=len(table), tok_bias=T(table), bias_of=T(np.full(len(bias_of), -1, np.int32)))
        rig.held['bias_of'] = T(np.asarray(bias_of, np.int32))
        rig.args.bias_of = rig.held['bias_of'].data_ptr()
    else:
        ops.block_set(rig.args, rig.held, n_biases=len(table), tok_bias=T(table), bias_of=T(np.asarray(bias_of, np.int32)))
    return rig


def bias_row(table, bias_of, r):
    return table[bias_of[r]] if 0 <= bias_of[r] < len(table) else None


# ------------------------------------------------------------------------------------------------ 1. bias, bit for bit
@pytest.mark.parametrize('extras', [False, True], ids=['bias', 'bias+ban+temp+top_p'])
@pytest.mark.parametrize('V', [33, 327, 1024])
@pytest.mark.parametrize('kind', KINDS)
def test_a_biased_launch_is_the_unbiased_launch_on_float32_sums(kind, V, extras):
    if kind in (TXL, TXLQ) and V == 327:
        V = 200
    queue, guided = kind in (TXLQ, ACCQ), kind in (TXL, ACC)
    n, m = (4, 3) if queue else (3, 3)
    top = 7
    seed = 77 * kind + V + int(extras)
    rs = np.random.RandomState(seed)
    table = (rs.randn(3, V) * 2).astype(np.float32)
    inf_ids = [top, 3, V - 1]
    table[1, inf_ids] = -np.inf                                    # row 1: three entries that act as a ban
    # (row 2, another random row: never the row a draw may use - a guided follower's own entry names it, and the leader's row holds)
    n_b = len(table)
    # stream 0 row 0; stream 1 no bias (n_biases, a value outside the table, or -1); stream 2 row 1 (guided kinds: the follower of stream 0, whose
    # own entry names row 2 and is not used); job 3 of a queue -1
    none = -1 if extras else n_b                                   # both spellings of "no bias" reach every kind
    bias_of = [0, none, 2 if guided else 1, -1][:n]
    used = [0, none, 0 if guided else 1, -1][:n]                    # the row each stream's draw runs under
    bans = [[top + 1, 20], None, [top + 1, 20] if guided else [5], None][:n] if extras else [None] * n
    ctl = {}
    if extras:
        uniq = [[top + 1, 20], [5]]
        ctl = dict(tok_mask=np.stack([pack(b, V) for b in uniq]), mask_of=np.array([uniq.index(b) if b else -1 for b in bans], np.int32),
                   temp_of=np.array([0.8, 1.2, 0.8 if guided else 1.6, 1.0][:n], np.float32),
                   top_p_of=np.array([0.9, 0.97, 0.9 if guided else 0.6, 0.8][:n], np.float32))
    scale = np.float32(1.5)

    def rig():
        g = Rig(kind, V, n, m, seed=seed)
        g.params[0, 1] = 4                                         # MAX_EVENTS: stream 0 is DONE once LEN > 4 (a queue then admits its last job)
        if guided:
            g.params[2], g.U[:, 2] = g.params[0], g.U[:, 0]        # (b below has no pair: the follower's own column holds the leader's uniforms)
        if kind == WIN:
            g.rows = [2, 0, 1]
        return g

    a = set_bias(rig().build(**ctl), table, bias_of, raw=True)
    b = rig().build(**ctl)
    if guided:
        hc._ops().block_set(a.args, a.held, guide_cond=T(np.array([0, -1, 0], np.int32)), guide_uncond=T(np.array([2, -1, 2], np.int32)),
                            guide_scale=T(np.array([scale, 0, scale], np.float32)))
    c = None
    if not extras:                                                 # the -inf entries of row 1 as a ban, the rest of the row as the bias
        finite = table.copy()
        finite[1, inf_ids] = 0.0
        who = [r for r in range(n) if used[r] == 1]
        if who:
            c = set_bias(rig().build(tok_mask=np.stack([pack(inf_ids, V)]), mask_of=np.array([0 if r in who else -1 for r in range(n)], np.int32)),
                         finite, bias_of, raw=True)
    drew = ended = redrew = 0
    for step in range(14):
        logits = a.batch(rs)
        logits[:, top] = logits.max(axis=1) + 1.0
        logits[:, a.pad] = logits[:, top] + (3.0 if step in (5, 6) else -2.0)      # (two launches in which PAD is the likeliest draw)
        ref = logits.copy()
        # (b's own slots: which free slot of a queue gets which job is not specified, and a sees the same raw row in every slot)
        for row, r in enumerate(b.stream_of_row()):
            if not 0 <= r < n:
                continue
            l = logits[row]
            if guided and r in (0, 2):
                lc, lu = logits[0], logits[2]
                l = lc + scale * (lc - lu)                         # three float32 operations, each rounded
            br = bias_row(table, used, r)
            ref[row] = l if br is None else l + br                 # NumPy float32: one rounded add
        s0 = a.t['state'].cpu().numpy().copy()
        a.launch(logits)
        b.launch(ref)
        sa, sb = a.snap(), b.snap()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (step, k, sa[k].tolist(), sb[k].tolist())
        if c is not None:
            c.launch(logits)
            sc = c.snap()
            for k in sa:
                assert np.array_equal(sa[k], sc[k]), ('ban', step, k)
        s1, seq = sa['state'], sa['seq']
        redrew += int((s1[:, S_DRAWS[kind]] - s0[:, S_DRAWS[kind]] > 1).sum())
        ended += int(((s1[:, 0] != 0) & (s0[:, 0] == 0)).sum())
        for r in range(n):
            if s1[r, S_ACCEPTED[kind]] > s0[r, S_ACCEPTED[kind]]:
                drew += 1
                tok = int(seq[r, s0[r, S_LEN]])
                assert not (used[r] == 1 and tok in inf_ids), (step, r, tok)
                assert not (bans[r] and tok in bans[r]), (step, r, tok)
        if guided:
            assert np.array_equal(seq[0, 2:], seq[2, 2:]), step    # the follower stays token for token with its leader
    assert drew >= 8 and ended >= 1
    if kind in (ACC, WIN, ACCQ):
        assert redrew >= 1
    if queue:
        assert int(a.t['queue_head'].item()) >= n


def test_the_txl_key_draw_runs_under_the_bias_and_the_cuts():
    V, n, key = 200, 3, 20

    def rig():
        g = Rig(TXL, V, n, L=1, seed=9)
        g.flags[:] = 0
        g.params[:, 3] = 1                                         # KEYED: with LEN == 1 the next draw is the key draw
        g.state[:, 6] = 1
        return g

    rs = np.random.RandomState(4)
    logits = (rs.randn(n, V) * 2).astype(np.float32)
    table = np.zeros((1, V), np.float32)
    table[0, key] = 60.0
    a = set_bias(rig().build(), table, [0, -1, 0])
    b = rig().build()
    k1 = rig().build(top_k_of=np.array([1, 0, 1], np.int32))
    mp = rig().build(min_p_of=np.array([1.5, 0, 2.0], np.float32))
    for g in (a, b, k1, mp):
        g.launch(logits)
    sa, sb = a.snap()['seq'], b.snap()['seq']
    assert sa[[0, 2], 1].tolist() == [key, key] and sa[1, 1] == sb[1, 1]
    arg = logits.argmax(axis=1)
    for g in (k1, mp):
        s = g.snap()['seq']
        assert s[[0, 2], 1].tolist() == arg[[0, 2]].tolist() and s[1, 1] == sb[1, 1]


# ------------------------------------------------------------------------------------------------ 2. the cuts against the float64 restatement
def _gap_top_p(sp, j):
    """A top_p in the middle between the two consecutive prefixes cum[j] and cum[j + 1]: far from both."""
    cum = np.cumsum(sp)
    return float(np.float32(0.5 * (cum[j] + cum[j + 1])))


def _gap_min_p(sp, lo, hi):
    """A min_p whose threshold lies in the (relatively) widest gap between sp[j] and sp[j + 1], lo <= j < hi."""
    j = lo + int(np.argmax(sp[lo:hi] / sp[lo + 1:hi + 1]))
    return float(np.float32(np.sqrt(sp[j] * sp[j + 1]) / sp[0]))


def _cases(V, rng):
    """-> [(logits row, temp, top_p, top_k, min_p)] with the margins asserted: no prefix within nucleus_ref's rounding bound of top_p, no
    probability within a relative 1e-4 of the min_p threshold."""
    out = []
    ks = [1, 2, 5, 17, V, V + 5, 0]
    for trial in range(6):
        scale, temp = (4.0, 1.1) if trial % 2 else (2.0, 1.2)
        row = nr.family_rows(rng, V, scale, 1)[0]
        sp = np.sort(nr.probs64(row, temp))[::-1]
        top_p = _gap_top_p(sp, 2 + 3 * trial)
        n_lo, n_hi = nr.cut_bracket(sp, top_p, V)
        assert n_lo == n_hi and 3 <= n_lo < V, (V, trial, n_lo, n_hi)
        for mode in ('k', 'm', 'both'):
            k = ks[(trial + len(out)) % len(ks)] if mode != 'm' else 0
            if mode == 'k' and k == 0:
                k = 3
            m = _gap_min_p(sp, 0, min(V - 2, 12)) if mode != 'k' else 0.0
            if m > 0:
                thr = np.float64(np.float32(m)) * sp[0]
                assert (np.abs(sp - thr) > 1e-4 * thr).all(), (V, trial, m)
            out.append((row, temp, top_p, k, m))
    return out


def _probes(row, temp, top_p, k, m):
    """Uniforms at which no CDF boundary lies within rounding: u = 0, and the float32 midpoints of the first, a middle and the last interval
    of the final candidate set that is wider than 2 DELTA (asserted: the first and the widest always are)."""
    from emo_disentanger_amd import sampling
    sp = np.sort(nr.probs64(row, temp))[::-1]
    count = sampling.soft_cut_count(sp, nr.cut_count(np.cumsum(sp), top_p, len(sp)), k, float(np.float32(m)))
    cdf = np.cumsum(sp[:count]) / sp[:count].sum()
    width = np.diff(cdf, prepend=0.0)
    wide = [i for i in range(count) if width[i] > 2 * nr.DELTA]
    assert wide and wide[0] == 0
    pick = sorted({wide[0], wide[len(wide) // 2], wide[-1]})
    return count, [np.float32(0)] + [np.float32(cdf[i] - 0.5 * width[i]) for i in pick]


def _launch_rows(kind, rows, temps, top_ps, ks, ms, us):
    """One launch: stream r draws from rows[r] at us[r] under its own temp / top_p / top_k / min_p; every draw is accepted -> the ids."""
    R, V = len(rows), len(rows[0])
    rig = Rig(kind, V, R, L=2, width=16, n_u=1)
    rig.flags[:] = 0
    rig.U = np.array(us, np.float32).reshape(1, R)
    rig.state[:, 6 if kind == TXL else 2] = 2                      # the primer is fed: this launch draws
    rig.build(temp_of=np.array(temps, np.float32), top_p_of=np.array(top_ps, np.float32), top_k_of=np.array(ks, np.int32),
              min_p_of=np.array(ms, np.float32))
    rig.launch(np.stack(rows))
    st, seq = rig.t['state'].cpu().numpy(), rig.t['seq'].cpu().numpy()
    assert (st[:, S_LEN] == 3).all()
    return seq[:, 2].tolist()


@pytest.mark.parametrize('V', [33, 200, 327, 1024])
@pytest.mark.parametrize('kind', [TXL, ACC])
def test_ids_drawn_under_the_cuts_are_the_float64_restatements(kind, V):
    from emo_disentanger_amd import sampling
    rng = np.random.default_rng(31 * V + kind)
    rows, temps, top_ps, ks, ms, us, want, cut = [], [], [], [], [], [], [], 0
    for row, temp, top_p, k, m in _cases(V, rng):
        count, probes = _probes(row, temp, top_p, k, m)
        plain = nr.cut_count(np.cumsum(np.sort(nr.probs64(row, temp))[::-1]), top_p, V)
        cut += int(count < plain)
        for u in probes:
            rows.append(row), temps.append(temp), top_ps.append(top_p), ks.append(k), ms.append(m), us.append(u)
            want.append(sampling.draw_at(row, temp, top_p, u, top_k=k, min_p=m))
    assert cut >= 6                                                # the cuts bite
    got = _launch_rows(kind, rows, temps, top_ps, ks, ms, us)
    assert got == want, [(i, g, w, ks[i], ms[i], float(us[i])) for i, (g, w) in enumerate(zip(got, want)) if g != w]


@pytest.mark.parametrize('kind', [TXL, ACC, WIN])
def test_the_cut_edges_on_the_device(kind):
    V = 33
    base = (-0.25 * np.arange(V)).astype(np.float32)               # strictly descending: rank = index
    tie3 = base.copy()
    tie3[[4, 9, 20]] = 3.0                                         # three exact ties on top
    flat = (-1e-3 * np.arange(V)).astype(np.float32)               # cum[V - 2] < 0.985 < cum[V - 1]: a single crossing, all V kept
    um = nr.U_MAX
    # (row, temp, top_p, k, m, u, expected id)
    cases = [
        (tie3, 1.0, 0.9, 1, 0.0, um, 4), (tie3, 1.0, 0.9, 1, 0.0, 0.0, 4),         # k = 1: the arg-max under the tie rule, whatever u
        (tie3, 1.0, 0.9, 2, 0.0, 0.0, 4), (tie3, 1.0, 0.9, 2, 0.0, 0.49, 4),       # ties across k = 2: the two lowest indices, half each
        (tie3, 1.0, 0.9, 2, 0.0, 0.51, 9), (tie3, 1.0, 0.9, 2, 0.0, um, 9),
        (tie3, 1.0, 0.9, 0, 1.0, um, 20),                                          # min_p = 1: the whole tie group and nothing else
        (base, 1.0, 0.9, 0, 1.5, um, 0), (base, 1.0, 0.9, 5, 7.0, um, 0),          # min_p > 1: the best token alone
        (base, 1.0, 2.0, 0, 0.0, um, 2), (base, 1.0, 2.0, 2, 0.0, um, 1),          # no crossing: top 3, cut to 2 by k
        (base, 1.0, 2.0, 0, 0.7, um, 1),                                           # ... and by min_p: exp(-0.25) = 0.78 >= 0.7 > exp(-0.5)
        (flat, 1.0, 0.985, 0, 0.0, um, V - 1), (flat, 1.0, 0.985, 5, 0.0, um, 4),  # single crossing: all V, cut to 5 by k
        (flat, 1.0, 0.985, 0, 0.99, um, 10),                                       # ... and by min_p: exp(-0.010) >= 0.99 > exp(-0.011)
        (base, 1.0, 0.9, V, 0.0, 0.0, 0), (base, 1.0, 0.9, V + 9, 0.0, 0.0, 0), (base, 1.0, 0.9, -3, -1.0, 0.0, 0),      # off
    ]
    from emo_disentanger_amd import sampling
    for row, temp, top_p, k, m, u, want in cases:
        assert sampling.draw_at(row, temp, top_p, u, top_k=k, min_p=m) == want, (k, m, u)
    rows, temps, top_ps, ks, ms, us, want = (list(x) for x in zip(*cases))
    if kind == WIN:                                                # (the windowed launch: the same draw through emo_nucleus_pick's other caller)
        R = len(rows)
        rig = Rig(WIN, V, R, L=2, width=16, n_u=1)
        rig.flags[:] = 0
        rig.U = np.array(us, np.float32).reshape(1, R)
        rig.build(temp_of=np.array(temps, np.float32), top_p_of=np.array(top_ps, np.float32), top_k_of=np.array(ks, np.int32),
                  min_p_of=np.array(ms, np.float32))
        rig.launch(np.stack(rows))
        got = rig.t['seq'].cpu().numpy()[:, 2].tolist()
    else:
        got = _launch_rows(kind, rows, temps, top_ps, ks, ms, us)
    assert got == want


# ------------------------------------------------------------------------------------------------ 3. scores
@pytest.mark.parametrize('kind', KINDS)
def test_the_scores_under_the_soft_controls_are_the_models_from_the_unbiased_row(kind):
    ops = hc._ops()
    V = 327
    queue = kind in (TXLQ, ACCQ)
    n, m = (4, 3) if queue else (3, 3)
    top = 7
    table = np.zeros((1, V), np.float32)
    table[0, top] = -30.0                                          # the model's favourite is (all but) never drawn
    table[0, 50:60] = 4.0
    g = Rig(kind, V, n, m, seed=3).build(scores=True, top_k_of=np.full(n, 12, np.int32), min_p_of=np.full(n, 0.02, np.float32))
    set_bias(g, table, [0] * n)
    rs = np.random.RandomState(8)
    hits = []
    for step in range(8):
        logits = g.batch(rs)
        logits[:, top] = logits.max(axis=1) + 1.0
        s0 = g.t['state'].cpu().numpy().copy()
        of_row = g.stream_of_row()
        g.launch(logits)
        s1, seq = g.t['state'].cpu().numpy(), g.t['seq'].cpu().numpy()
        for r in range(n):
            if s1[r, S_ACCEPTED[kind]] > s0[r, S_ACCEPTED[kind]]:
                c = int(s0[r, S_LEN])
                hits.append((r, c, int(seq[r, c]), logits[of_row.index(r)]))
    assert len(hits) >= 8
    lp, rk, en = (g.tabs[k].cpu().numpy() for k in TABLES)
    cells = np.zeros((n, g.width), bool)
    ts = ops.token_scores(T(np.stack([h[3] for h in hits])), torch.tensor([h[2] for h in hits], device=DEV), -100, want=('rank', 'entropy'))
    nll, rank, ent = ts['nll'].cpu().numpy(), ts['rank'].cpu().numpy(), ts['entropy'].cpu().numpy()
    for i, (r, c, tok, row) in enumerate(hits):
        assert tok != top
        cells[r, c] = True
        logp, rank64, ent64 = hc.ref_scores(row, tok)              # the unbiased row: the banned-by-bias arg-max still counts
        assert rk[r, c] == rank[i] == rank64 and rank64 >= 1
        assert abs(float(lp[r, c]) + float(nll[i])) <= 2 * row_tol(row) and abs(float(en[r, c]) - float(ent[i])) <= 2 * row_tol(row)
        assert abs(float(lp[r, c]) - logp) <= row_tol(row) and abs(float(en[r, c]) - ent64) <= row_tol(row)
    assert np.array_equal(rk >= 0, cells) and np.array_equal(~np.isnan(lp), cells)


# ------------------------------------------------------------------------------------------------ 4. all fields NULL
NEW = ('tok_bias', 'bias_of', 'top_k_of', 'min_p_of')


@pytest.mark.parametrize('kind', KINDS)
def test_with_every_soft_field_null_the_block_is_the_one_without_them(kind):
    queue = kind in (TXLQ, ACCQ)
    n, m = (4, 3) if queue else (3, 3)
    a = Rig(kind, 200, n, m, seed=5).build(scores=True)
    b = Rig(kind, 200, n, m, seed=5).build(scores=True, **{k: None for k in NEW})
    for k in NEW:
        assert getattr(a.args, k) is None and getattr(b.args, k) is None
    assert a.args.n_biases == 0
    b.args.n_biases = 5                                            # without tok_bias the count is not read
    rs = np.random.RandomState(6)
    for step in range(8):
        logits = a.batch(rs)
        a.launch(logits)
        b.launch(logits)
        sa, sb = a.snap(), b.snap()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (step, k)
    for k in TABLES:
        assert np.array_equal(hc._bits(a.tabs[k]), hc._bits(b.tabs[k]))
    assert int((a.tabs['tok_rank'] >= 0).sum().item()) >= 8
