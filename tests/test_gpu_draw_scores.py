"""GPU: the per-token outputs of emo_grammar_step (tok_logp / tok_rank / tok_entropy, emo_draw_scores.h) — the figures of every ACCEPTED draw
against a float64 restatement on the same fp32 logits row and against emo_token_scores, that no other cell of the tables is ever written
(primer, injected bar, rejected draws, every ending), and that the launch does what it did without them.  The three kinds are driven
directly, on small synthetic event tables: every id is a plain event except the ones a case names."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-5          # absolute, per row: the bound tests/test_gpu_token_scores.py holds emo_token_scores to at the logit scale randn x 3
                        # (values below 16 in magnitude: one fp32 ulp there is 2^-20 ~ 1e-6, so the bound is ~10 ulp of the largest logit)
ULP16 = float(np.spacing(np.float32(15.99)))
TXL, ACC, WIN = 0, 1, 2
S_LEN = 1
S_ACCEPTED = {TXL: 2, ACC: 7, WIN: 7}
TABLES = ('tok_logp', 'tok_rank', 'tok_entropy')
FILL = {'tok_logp': 0x7FC00001, 'tok_rank': -1, 'tok_entropy': 0x7FC00002}       # the caller's bit patterns: two NaNs and -1
DEV = 'cuda'


def _ops():
    from emo_disentanger_amd import ops
    return ops


def row_tol(row):
    """ROW_TOL, scaled by the ulp of the row's largest |logit| where that is above the scale ROW_TOL was derived at."""
    return ROW_TOL * max(1.0, float(np.spacing(np.float32(np.abs(row).max()))) / ULP16)


def ref_scores(row, tok):
    """float64 from the same fp32 values: (logp, rank, entropy) of `tok` at temperature 1."""
    l = row.astype(np.float64)
    mx = l.max()
    lse = mx + np.log(np.exp(l - mx).sum())
    p = np.exp(l - lse)
    return l[tok] - lse, int((l > l[tok]).sum() + (l[:tok] == l[tok]).sum()), lse - float((p * l).sum())


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def make_tables(n, width, which=TABLES):
    return {k: torch.full((n, width), FILL[k], dtype=torch.int32, device=DEV).view(torch.int32 if k == 'tok_rank' else torch.float32) for k in which}


def bits(t):
    return t.view(torch.int32).cpu().numpy().copy()


class Rig:
    """n streams of one kind on the device.  Plain streams: RUNNING, a primer of L tokens already fed, the next launch draws.  Fields of
    `state` / `params` / `flags` / `beat` / `U` may be changed (numpy) before build()."""

    def __init__(self, kind, V, n, L=3, width=24, n_u=64, seed=0):
        self.kind, self.V, self.n, self.L, self.width, self.n_u = kind, V, n, L, width, n_u
        rs = np.random.RandomState(seed)
        self.flags, self.beat = np.zeros(V, np.int32), np.zeros(V, np.int32)
        self.pad = V - 1
        self.flags[self.pad] = 4                                   # EMO_TXL_EV_PAD == EMO_ACC_EV_PAD
        self.U = rs.rand(n_u, n).astype(np.float32)
        self.seq = np.zeros((n, width), np.int64)
        self.seq[:, :L] = rs.randint(0, max(1, V - 1), (n, L))
        self.segs = np.zeros((n, width), np.int64)
        self.params, self.state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
        if kind == TXL:
            self.params[:, :3] = 1000, 1000, L                     # MAX_BARS, MAX_EVENTS, PRIMER_LEN
            self.state[:, S_LEN], self.state[:, 6] = L, L          # LEN, FEED
        else:
            self.params[:, :5] = 50, 1000, 0, 0, 1                 # TARGET_BARS, MAX_EVENTS, SKIP_CHECK, BAR0, N_BARS
            self.state[:, S_LEN], self.state[:, 2] = L, L          # LEN, CONSUMED
        self.lead_tok, self.lead_off = np.zeros(4, np.int64), np.array([0, 2, 4], np.int32)
        self.max_len, self.window, self.track_full = width + 8, 2, 0
        self.temperature, self.top_p, self.key_temperature, self.key_top_p = 1.2, 0.9, 1.1, 0.97

    def build(self, which=TABLES, rows=None, m=None):
        ops = _ops()
        n, V = self.n, self.V
        self.m = m = (len(rows) if rows is not None else n) if m is None else m
        self.rows = rows
        self.t = dict(u_steps=T(self.U), ev_flags=T(self.flags), ev_beat=T(self.beat), params=T(self.params), state=T(self.state), seq=T(self.seq),
                      running=torch.tensor([int((self.state[:, 0] == 0).sum())], dtype=torch.int32, device=DEV))
        self.logits = torch.zeros(m, V, device=DEV)
        num = dict(n_rows=m, n_token=V, ld_u=n, temperature=self.temperature, top_p=self.top_p)
        if self.kind == TXL:
            num.update(key_temperature=self.key_temperature, key_top_p=self.key_top_p)
            self.t.update(tok_out=torch.full((n,), -1, dtype=torch.long, device=DEV))
        else:
            num.update(track_full=self.track_full)
            self.t.update(segs=T(self.segs), lead_tok=T(self.lead_tok), lead_off=T(self.lead_off))
            if self.kind == ACC:
                num.update(max_len=self.max_len, pad=self.pad)
                self.t.update(tok_out=torch.full((n,), -1, dtype=torch.long, device=DEV), seg_out=torch.full((n,), -1, dtype=torch.long, device=DEV))
            else:
                num.update(window=self.window)
                self.t.update(win_tok=torch.full((m, self.window), -1, dtype=torch.long, device=DEV),
                              win_seg=torch.full((m, self.window), -1, dtype=torch.long, device=DEV))
                if rows is not None:
                    self.t.update(rows=torch.tensor(rows, dtype=torch.int32, device=DEV))
        self.tabs = make_tables(n, self.width, which)
        self.args, self.held = ops.GrammarStep(kind=self.kind), {}
        ops.block_set(self.args, self.held, logits=self.logits, **num, **self.t, **self.tabs)
        return self

    def stream_row(self):
        """stream -> its row of the logits batch"""
        if self.kind != WIN or self.rows is None:
            return {r: r for r in range(self.m)}
        return {r: b for b, r in enumerate(self.rows)}

    def launch(self, logits):
        """One launch on `logits` (numpy [m, V]); -> [(stream, column, token)] of the draws accepted in it, after checking that exactly their
        cells changed and that they hold the float64 figures of their logits rows."""
        ops = _ops()
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        self.logits.copy_(T(logits))
        st0 = self.t['state'].cpu().numpy().copy()
        tab0 = {k: bits(v) for k, v in self.tabs.items()}
        ops.grammar_step(self.args)
        torch.cuda.synchronize()
        st1, seq = self.t['state'].cpu().numpy(), self.t['seq'].cpu().numpy()
        tab1 = {k: bits(v) for k, v in self.tabs.items()}
        got = {k: v.cpu().numpy() for k, v in self.tabs.items()}
        acc_w = S_ACCEPTED[self.kind]
        row_of = self.stream_row()
        hits = []
        for r in range(self.n):
            d = int(st1[r, acc_w]) - int(st0[r, acc_w])
            assert d in (0, 1), (r, st0[r].tolist(), st1[r].tolist())
            assert d == 0 or r in row_of
            if d:
                c = int(st0[r, S_LEN])
                tok = int(seq[r, c])
                row = logits[row_of[r]]
                logp, rank, ent = ref_scores(row, tok)
                tol = row_tol(row)
                if 'tok_rank' in got:
                    assert got['tok_rank'][r, c] == rank, (r, c, tok, got['tok_rank'][r, c], rank)
                if 'tok_logp' in got:
                    e = abs(float(got['tok_logp'][r, c]) - logp)
                    assert e <= tol, 'logp of stream %d col %d: err %.3e (bound %.1e)' % (r, c, e, tol)
                if 'tok_entropy' in got:
                    e = abs(float(got['tok_entropy'][r, c]) - ent)
                    assert e <= tol, 'entropy of stream %d col %d: err %.3e (bound %.1e)' % (r, c, e, tol)
                for k in tab0:
                    tab0[k][r, c] = tab1[k][r, c]                   # the one cell that may differ
                hits.append((r, c, tok))
        for k in tab0:
            assert np.array_equal(tab0[k], tab1[k]), (k, np.argwhere(tab0[k] != tab1[k]).tolist())
        return hits

    def written(self, k):
        """per stream: the columns of table k that no longer hold the caller's pattern"""
        b = bits(self.tabs[k])
        return [np.flatnonzero(b[r] != np.int32(FILL[k])).tolist() for r in range(self.n)]


# ------------------------------------------------------------------------------------------------ 1. the figures
@pytest.mark.parametrize('V', [3, 200, 327, 1024])
@pytest.mark.parametrize('kind', [TXL, ACC, WIN])
def test_the_figures_of_accepted_draws_match_float64_and_emo_token_scores(kind, V):
    # stream 0 and 1: fresh randn x 3 rows every step, once shifted by +80 / -80 (the max shift; the bound follows the ulp of the largest logit);
    # stream 2: three equal dominant logits at t - 1, t, t + 1 and the uniform 0.5, which picks the middle one: exact ties below and above the
    # accepted index, rank exactly 1.  V = 3 has PAD (id 2) drawn about every third time: redrawn inside the launch (ACC, ACC_WINDOW), rejected (TXL).
    ops = _ops()
    rig = Rig(kind, V, 3, seed=V + kind)
    rig.U[:, 2] = 0.5
    rig.build()
    rs = np.random.RandomState(100 + V)
    t = 1 if V == 3 else V // 2
    hits, tie_hits = [], 0
    for step in range(5):
        logits = (rs.randn(3, V) * 3).astype(np.float32)
        if step == 1:
            logits[0] += 80.0
            logits[1] -= 80.0
        logits[2, t - 1:t + 2] = logits[2].max() + 8.0
        for r, c, tok in rig.launch(logits):                       # (launch() holds every hit to float64)
            hits.append((r, c, tok, logits[rig.stream_row()[r]]))
            if r == 2:
                assert tok == t and rig.tabs['tok_rank'][2, c].item() == 1
                tie_hits += 1
    assert len(hits) >= 6 and tie_hits == 5
    # against emo_token_scores on the same rows, tgt = the accepted ids: ranks equal, nll within 2 x the row's bound
    ts = ops.token_scores(T(np.stack([h[3] for h in hits])), torch.tensor([h[2] for h in hits], device=DEV), -100, want=('rank', 'entropy'))
    nll, rank = ts['nll'].cpu().numpy(), ts['rank'].cpu().numpy()
    lp, rk = rig.tabs['tok_logp'].cpu().numpy(), rig.tabs['tok_rank'].cpu().numpy()
    for i, (r, c, tok, row) in enumerate(hits):
        assert rk[r, c] == rank[i], (r, c, tok)
        assert abs(float(lp[r, c]) + float(nll[i])) <= 2 * row_tol(row), (r, c, float(lp[r, c]), float(nll[i]))


# ------------------------------------------------------------------------------------------------ 2. exactly the drawn cells
@pytest.mark.parametrize('kind', [TXL, ACC, WIN])
def test_exactly_the_drawn_cells_are_written(kind):
    # stream 0 still feeds its primer (TXL, ACC: two tokens longer than the common prefix), stream 1 draws Track_LeadSheet first and gets a
    # lead-sheet bar and Track_Full injected (ACC, ACC_WINDOW), stream 2 is plain.  After 8 launches: the cells written are the columns of the
    # accepted draws and nothing else — not the primer, not the injected bar, not the columns past LEN — and there are state[ACCEPTED] of them.
    V = 40
    rig = Rig(kind, V, 3, L=3, width=32, seed=7)
    tls, tfull, bar = 30, 31, [32, 33]
    if kind != TXL:
        rig.flags[tls] = 2                                         # EMO_ACC_EV_TRACK_LS
        rig.track_full = tfull
        rig.lead_tok, rig.lead_off = np.array([5, 6] + bar, np.int64), np.array([0, 2, 4], np.int32)
        rig.params[:, 0], rig.params[:, 4] = 3, 2                  # TARGET_BARS 3, N_BARS 2: one injection, then the bar table is exhausted
    if kind == TXL:
        rig.seq[0, :5] = [1, 2, 3, 4, 5]
        rig.params[0, 2], rig.state[0, S_LEN] = 5, 5               # PRIMER_LEN, LEN; FEED stays 3
    elif kind == ACC:
        rig.seq[0, :5] = [1, 2, 3, 4, 5]
        rig.state[0, S_LEN] = 5                                    # CONSUMED stays 3
    rig.build()
    rs = np.random.RandomState(3)
    drawn = {r: [] for r in range(3)}
    for step in range(8):
        logits = (rs.randn(3, V) * 3).astype(np.float32)
        logits[:, [tls, tfull] + bar] = -30.0
        if kind != TXL and step == 0:
            logits[1, tls] = 30.0
        for r, c, tok in rig.launch(logits):
            drawn[r].append(c)
    st, seq = rig.t['state'].cpu().numpy(), rig.t['seq'].cpu().numpy()
    assert (st[:, 0] == 0).all()                                   # all still RUNNING
    for k in TABLES:
        w = rig.written(k)
        for r in range(3):
            assert w[r] == drawn[r], (k, r, w[r], drawn[r])
            assert len(w[r]) == st[r, S_ACCEPTED[kind]]
            assert all(c < st[r, S_LEN] for c in w[r])
    first = 5 if kind != WIN else 3
    assert drawn[0] and min(drawn[0]) == first                     # nothing inside the primer
    if kind != TXL:
        assert seq[1, 3:7].tolist() == [tls] + bar + [tfull] and drawn[1][0] == 3 and all(c >= 7 for c in drawn[1][1:])
        assert len(drawn[1]) >= 2


# ------------------------------------------------------------------------------------------------ 3. rejections and endings
def _acc_endings(kind):
    """Streams 0..4 of an ACC-like rig and the logits of their one launch:
    0 PAD dominant, first uniform picks it, the second the other word; 1 a Beat below the position, then one above; 2 the 256th rejected
    Beat -> STUCK; 3 PAD on the last uniform -> OUT_OF_DRAWS; 4 a full row -> OVERFLOW."""
    V, width, n_u = 50, 16, 8
    rig = Rig(kind, V, 5, L=3, width=width, n_u=n_u, seed=11)
    lo, hi, word = 20, 21, 10
    rig.flags[[lo, hi]] = 1
    rig.beat[lo], rig.beat[hi] = 2, 8
    rig.state[[1, 2], 4] = 5                                       # CUR_POS
    rig.state[2, 5] = 255                                          # FAILED
    rig.state[3, 6] = n_u - 1                                      # DRAWS
    rig.state[4, S_LEN] = width
    if kind == ACC:
        rig.state[4, 2] = width                                    # CONSUMED
    rig.U[:, :] = 0.2
    rig.U[1, [0, 1]] = 0.95, 0.8
    logits = np.full((5, V), -20.0, np.float32)
    logits[0, rig.pad], logits[0, word] = 5.0, 3.0
    logits[1, [lo, hi]] = 6.0
    logits[2, lo] = 9.0
    logits[3, rig.pad] = 9.0
    logits[4, word] = 9.0
    return rig, logits, (lo, hi, word)


def test_acc_rejections_record_the_accepted_word_only_and_endings_record_nothing():
    from emo_disentanger_amd import inference as inf
    rig, logits, (lo, hi, word) = _acc_endings(ACC)
    rig.build()
    hits = rig.launch(logits)
    st = rig.t['state'].cpu().numpy()
    assert hits == [(0, 3, word), (1, 3, hi)]
    assert st[:, 0].tolist() == [inf.ACC_RUNNING, inf.ACC_RUNNING, inf.ACC_STUCK, inf.ACC_OUT_OF_DRAWS, inf.ACC_OVERFLOW]
    assert st[0, 6] == 2 and st[1, 6] == 2 and st[1, 5] == 0       # two draws each; the accepted Beat reset the count
    rk = rig.tabs['tok_rank'].cpu().numpy()
    assert rk[0, 3] == 1 and rk[1, 3] == 1                         # behind PAD; the second of two equal logits
    for k in TABLES:
        assert rig.written(k) == [[3], [3], [], [], []]
    # WINDOW: every stream still running is at max_len in the next launch and records nothing
    ops = _ops()
    ops.block_set(rig.args, rig.held, max_len=3)
    assert rig.launch(logits) == []
    assert rig.t['state'].cpu().numpy()[:2, 0].tolist() == [inf.ACC_WINDOW] * 2
    for k in TABLES:
        assert rig.written(k) == [[3], [3], [], [], []]


def test_window_kind_records_through_the_rows_indirection_with_a_row_dropped():
    from emo_disentanger_amd import inference as inf
    rig, logits, (lo, hi, word) = _acc_endings(WIN)
    rows = [4, 0, 2, 1]                                            # stream 3 is not in the batch
    # the uniforms are indexed by the stream, the logits by the batch row
    rig.build(rows=rows)
    hits = rig.launch(logits[rows])
    st = rig.t['state'].cpu().numpy()
    assert hits == [(0, 3, word), (1, 3, hi)]
    assert st[:, 0].tolist() == [inf.ACC_RUNNING, inf.ACC_RUNNING, inf.ACC_STUCK, inf.ACC_RUNNING, inf.ACC_OVERFLOW]
    assert st[3].tolist() == rig.state[3].tolist()
    for k in TABLES:
        assert rig.written(k) == [[3], [3], [], [], []]
    wt = rig.t['win_tok'].cpu().numpy()
    assert wt[1].tolist() == [int(rig.seq[0, 2]), word] and wt[3].tolist() == [int(rig.seq[1, 2]), hi]


def test_txl_rejections_endings_and_the_key_draw_at_temperature_one():
    from emo_disentanger_amd import stage1_inference as s1
    V, n_u = 50, 8
    rig = Rig(TXL, V, 6, L=1, width=16, n_u=n_u, seed=13)
    lo, key, word = 20, 25, 10
    rig.flags[lo], rig.beat[lo] = 1, 2
    rig.flags[key] = 16 | 32                                       # a major key
    rig.seq[:, 1] = 7
    rig.state[[0, 2, 5], S_LEN] = 2                                # streams 1, 3, 4 hold one token: with KEYED their next draw is the key draw
    rig.state[0, 3] = 5                                            # BEAT: the drawn Beat_2 is below it -> rejected
    rig.state[2, 3], rig.state[2, 5] = 5, 255                      # ... the 256th in a row -> STUCK
    rig.params[[1, 3, 4], 3] = 1                                   # KEYED
    rig.params[[3, 4], 4] = 1                                      # KEY_RULE
    rig.params[3, 5] = 2                                           # EMO_MODE minor: a major key is rejected
    rig.state[5, 7] = n_u                                          # DRAWS: the table is used up -> OVERFLOW
    rig.key_temperature, rig.key_top_p = 3.0, 0.97
    rig.build()
    rs = np.random.RandomState(5)
    logits = np.full((6, V), -20.0, np.float32)
    logits[0, lo] = logits[2, lo] = 9.0
    logits[1] = (rs.randn(V) * 3).astype(np.float32)               # the key draw of a stream without the key rule: any word is accepted
    logits[1, rig.pad] = -20.0
    logits[3, key] = 9.0
    logits[4, word] = 9.0                                          # not a Key event under the key rule -> KEY_ERROR
    hits = rig.launch(logits)                                      # (checks the figures against float64 at temperature 1)
    st = rig.t['state'].cpu().numpy()
    assert [h[:2] for h in hits] == [(1, 1)]
    assert st[:, 0].tolist() == [s1.RUNNING, s1.RUNNING, s1.STUCK, s1.RUNNING, s1.KEY_ERROR, s1.OVERFLOW]
    assert st[0, 5] == 1 and st[3, 7] == 1 and st[3, S_LEN] == 1   # a counted Beat rejection; the rejected key draw was a draw
    for k in TABLES:
        assert rig.written(k) == [[], [1], [], [], [], []]
    # the same logits drawn at the key temperature are not the figures recorded: temperature 3 flattens the row
    lp = float(rig.tabs['tok_logp'][1, 1].item())
    l3 = logits[1].astype(np.float64) / 3.0
    lp3 = l3[hits[0][2]] - (l3.max() + np.log(np.exp(l3 - l3.max()).sum()))
    assert abs(lp - lp3) > 100 * ROW_TOL


# ------------------------------------------------------------------------------------------------ 4. behaviour unchanged
def _run(kind, which):
    V = 12
    rig = Rig(kind, V, 4, L=3, width=32, n_u=16, seed=21)
    rig.flags[[6, 7]] = 1
    rig.beat[6], rig.beat[7] = 1, 9                                # Beats: rejections
    rig.flags[5] = 8 if kind == TXL else 2                         # TXL: EOS -> DONE; else Track_LeadSheet: an injection, then the bar table ends
    if kind != TXL:
        rig.track_full = 4
        rig.lead_tok, rig.lead_off = np.array([1, 2, 3, 8], np.int64), np.array([0, 2, 4], np.int32)
        rig.params[:, 0], rig.params[:, 4] = 3, 2
    rig.state[3, 0] = 1                                            # a finished stream
    rig.build(which=which)
    rs = np.random.RandomState(17)
    snaps = []
    for step in range(10):
        logits = (rs.randn(4, V) * 2).astype(np.float32)
        logits[:, 5] += 2.0
        rig.launch(logits)
        snaps.append({k: v.cpu().numpy().copy() for k, v in rig.t.items() if k in ('seq', 'segs', 'state', 'tok_out', 'seg_out', 'win_tok', 'win_seg',
                                                                                    'running')})
    return snaps, {k: bits(v) for k, v in rig.tabs.items()}


@pytest.mark.parametrize('kind', [TXL, ACC, WIN])
def test_the_launch_is_unchanged_by_the_outputs_and_any_one_works_alone(kind):
    base, none = _run(kind, ())
    assert none == {}
    full, tabs = _run(kind, TABLES)
    assert any((t != np.int32(FILL[k])).any() for k, t in tabs.items())
    for a, b in zip(base, full):
        assert a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert len({tuple(s['state'][:, 0]) for s in base}) > 1        # something ended on the way
    for k in TABLES:
        one, tab = _run(kind, (k,))
        assert np.array_equal(tab[k], tabs[k])
        for a, b in zip(base, one):
            for f in a:
                assert np.array_equal(a[f], b[f]), (k, f)
