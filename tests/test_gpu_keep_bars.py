"""GPU: kept bars in the stage-2 grammar launch (emo_grammar_step, kinds ACC and ACC_QUEUE: keep_tok / keep_beg / keep_end), kernel level, on
hand-built rows and a small synthetic grammar, V = 33 and 327.  The logits of a drawing launch are peaked on one or two words, so that the
float64 sampler of tests/nucleus_ref.py gives the drawn id from the same uniform; the host side is inference._Stream (with keep) driven by those
ids.  After EVERY launch tok_out, seg_out, state, seq, segs and the running count equal the host's, bit for bit."""
import copy

import numpy as np
import pytest
import torch

import nucleus_ref as nr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TRACK_LS, TRACK_FULL, BEAT0, N_BEATS, PAD, EOS = 5, 6, 8, 16, 24, 25
TABLES = ('tok_logp', 'tok_rank', 'tok_entropy')
WIDTH, W, N_U = 64, 56, 64
BOOST = 60.0
PRIMER = [0, 3, 4]
LEAD = [[7, 26], [7, 27, 28], [7], [7, 29], [7, 30]]
BEAT = lambda k: BEAT0 + k          # noqa: E731
ROW_TOL = 1e-5                       # tests/test_gpu_draw_scores.py: absolute, per row, at |l| < 16; scaled below by the ulp of the row's largest |logit|
ULP16 = float(np.spacing(np.float32(15.99)))


def vocab(V):
    names = {TRACK_LS: 'Track_LeadSheet', TRACK_FULL: 'Track_Full', PAD: 'PAD_None', EOS: 'EOS_None'}
    names.update({BEAT0 + k: 'Beat_%d' % k for k in range(N_BEATS)})
    i2e = {i: names.get(i, 'Note_%d' % i) for i in range(V)}
    return {e: i for i, e in i2e.items()}, i2e


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def opened(bars):
    """The row length once bar `bars` has been opened behind `bars` empty bars (primer, then per bar Track_LeadSheet, lead bar, Track_Full)."""
    return len(PRIMER) + sum(len(LEAD[j]) + 2 for j in range(bars + 1))


# per stream: bars of LEAD, keep, max_events, uniforms {draw: u} (default 0.2: the lower id of two), the words boosted in each DRAWING launch
CASES = [
    # a drawn Track_LeadSheet followed by one kept bar (a kept Beat that goes back, a banned id and PAD's neighbour among its tokens)
    (3, [None, [1, BEAT(9), BEAT(2), 32], None], 1000, {}, [[31], [TRACK_LS], [30], [TRACK_LS]]),
    # ... by two consecutive kept bars
    (4, [None, [1], [2, 31], None], 1000, {}, [[TRACK_LS], [29], [TRACK_LS]]),
    # a kept empty bar
    (3, [None, [], None], 1000, {}, [[30], [TRACK_LS], [TRACK_LS]]),
    # a kept last bar: DONE with EOS
    (2, [None, [1, 2]], 1000, {}, [[31], [TRACK_LS]]),
    # a chain that does not fit ld_seq: OVERFLOW, nothing written
    (3, [None, [2], [1] * WIDTH], 1000, {}, [[29], [TRACK_LS]]),
    # max_events reached inside a kept bar
    (3, [None, [1, 2, 31, 32], None], opened(1) + 2, {}, [[TRACK_LS]]),
    # a Beat redraw in the launch that then accepts Track_LeadSheet before a kept bar (draw 1 picks Beat_2 < Beat_5: rejected; draw 2 Track_LeadSheet)
    (3, [None, [2], None], 1000, {1: 0.8}, [[BEAT(5)], [TRACK_LS, BEAT(2)], [TRACK_LS]]),
    # no kept bar in a block that has the tables: as ever
    (2, None, 1000, {}, [[31], [TRACK_LS], [TRACK_LS]]),
]
N = len(CASES)
WANT = [1, 1, 1, 1, 5, 1, 1, 1]                                     # DONE everywhere but the OVERFLOW


class Host:
    """One stream of the ACC launch on inference._Stream: HostAcc of tests/test_gpu_stage2_batch.py with keep, and the OVERFLOW of a bar opening."""

    def __init__(self, inf, e2i, i2e, lead, primer, keep, max_events, consumed, width=WIDTH, window=W):
        self.inf, self.e2i, self.i2e, self.max_events, self.width, self.W = inf, e2i, i2e, max_events, width, window
        self.s = inf._Stream(e2i, lead, primer, None, keep, max_events)
        self.s.consumed = consumed
        self.status = inf.ACC_DONE if self.s.done else inf.ACC_RUNNING
        self.draws = self.accepted = 0
        self.tok = self.seg = None
        self.cells = []                                             # where an accepted draw was appended

    def wants_draw(self):
        return self.status == self.inf.ACC_RUNNING and len(self.s.generated) < self.W and self.s.consumed == len(self.s.generated)

    def step(self, pick, n_u):
        inf, s = self.inf, self.s
        if self.status == inf.ACC_RUNNING and len(s.generated) >= self.W:
            self.status = inf.ACC_WINDOW
        elif self.status == inf.ACC_RUNNING and s.consumed == len(s.generated):
            while True:
                if self.draws >= n_u:
                    self.status = inf.ACC_OUT_OF_DRAWS
                    break
                w = pick(self.draws)
                self.draws += 1
                t = copy.deepcopy(s)
                ok = t.offer(w, self.e2i, self.i2e, False, self.max_events)
                if len(t.generated) > self.width:                   # the bar opening does not fit: the row and the counters as before the draw
                    assert w == TRACK_LS and s.keep is not None and s.keep[s.generated_bars + 1] is not None
                    self.draws -= 1
                    self.status = inf.ACC_OVERFLOW
                    break
                at = len(s.generated)
                self.s = s = t
                if s.stuck:
                    self.status = inf.ACC_STUCK
                    break
                if ok:
                    self.accepted += 1
                    self.cells.append(at)
                    if s.done:
                        self.status = inf.ACC_DONE
                    break
        if self.status == inf.ACC_RUNNING:
            self.tok, self.seg = s.generated[s.consumed], s.seg[s.consumed]
            s.consumed += 1
        else:
            self.tok, self.seg = PAD, 1

    def state(self):
        inf, s = self.inf, self.s
        d = {inf.ACC_S_STATUS: self.status, inf.ACC_S_LEN: len(s.generated), inf.ACC_S_BARS: s.generated_bars, inf.ACC_S_CUR_POS: s.cur_pos,
             inf.ACC_S_FAILED: s.failed_cnt, inf.ACC_S_DRAWS: self.draws, inf.ACC_S_ACCEPTED: self.accepted}
        if self.status == inf.ACC_RUNNING:
            d[inf.ACC_S_CONSUMED] = s.consumed
        return d


def ref_pick(row, ban, temp, top_p, u, V):
    """The id the reference sampler gives: tests/nucleus_ref.py's float64 softmax, order, cut and pick on the row under its ban."""
    row = np.array(row, np.float32)
    if ban:
        row[list(ban)] = -np.inf
    p = nr.probs64(row, temp)
    o = nr.order(p)
    n = nr.cut_count(np.cumsum(p[o]), top_p, V)
    return nr.expected_pick(o[:n], p, u)


class Rig:
    def __init__(self, V, cases=CASES, keep_tables=True, scores=False, controls=None, guide=None, seed=0):
        from emo_disentanger_amd import inference as inf, ops
        self.inf, self.V, self.cases, n = inf, V, cases, len(cases)
        self.e2i, self.i2e = vocab(V)
        self.controls, self.guide = controls, guide
        leads = [LEAD[:c[0]] for c in cases]
        keeps = [c[1] for c in cases]
        self.hosts = [Host(inf, self.e2i, self.i2e, leads[i], PRIMER, keeps[i], cases[i][2], len(PRIMER)) for i in range(n)]
        self.U = np.full((N_U, n), 0.2, np.float32)
        for i, c in enumerate(cases):
            for d, u in c[3].items():
                self.U[d, i] = u
        flags, beat = inf.acc_event_tables(self.i2e, V)
        toks, offs, bar0, nbars, _ = inf.pack_lead_sheets(leads)
        seq, segs = np.zeros((n, WIDTH), np.int64), np.zeros((n, WIDTH), np.int64)
        params, state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
        for i, h in enumerate(self.hosts):
            k = len(h.s.generated)
            seq[i, :k], segs[i, :len(h.s.seg)] = h.s.generated, h.s.seg
            params[i, :5] = h.s.target_bars, cases[i][2], 0, bar0[i], nbars[i]
            state[i, [inf.ACC_S_STATUS, inf.ACC_S_LEN, inf.ACC_S_CONSUMED, inf.ACC_S_BARS]] = h.status, k, len(PRIMER), h.s.generated_bars
        self.t = dict(u_steps=T(self.U), ev_flags=T(flags), ev_beat=T(beat), params=T(params), state=T(state), seq=T(seq), segs=T(segs),
                      lead_tok=T(toks), lead_off=T(offs), tok_out=torch.full((n,), -1, dtype=torch.long, device=DEV),
                      seg_out=torch.full((n,), -1, dtype=torch.long, device=DEV),
                      running=torch.tensor([sum(h.status == inf.ACC_RUNNING for h in self.hosts)], dtype=torch.int32, device=DEV))
        self.logits = torch.zeros(n, V, device=DEV)
        self.num = dict(n_rows=n, n_token=V, ld_u=n, temperature=1.2, top_p=0.9, track_full=TRACK_FULL, max_len=W, pad=PAD)
        more = {}
        if keep_tables:
            kt, kb, ke = inf.pack_keep(keeps, leads)
            self.num.update(n_keep=sum(len(b) for k in keeps if k for b in k if b is not None), keep_eos=EOS)
            more.update(keep_tok=T(kt), keep_beg=T(kb), keep_end=T(ke))
        if controls:
            self.num['n_masks'] = len(controls['tok_mask'])
            more.update({k: T(v.view(np.int32) if k == 'tok_mask' else v) for k, v in controls.items()})
        if guide:
            more.update({k: T(v) for k, v in guide.items()})
        self.tabs = {}
        if scores:
            self.tabs = {k: torch.full((n, WIDTH), -1 if k == 'tok_rank' else float('nan'), device=DEV,
                                       dtype=torch.int32 if k == 'tok_rank' else torch.float32) for k in TABLES}
        self.args, self.held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
        ops.block_set(self.args, self.held, logits=self.logits, **self.num, **self.t, **self.tabs, **more)
        self.launches, self.rs, self.drawn = [0] * n, np.random.RandomState(seed), []

    def ban_of(self, i):
        c = self.controls
        if not c or c['mask_of'][i] < 0:
            return []
        row = c['tok_mask'][c['mask_of'][i]]
        return [v for v in range(self.V) if row[v >> 5] >> np.uint32(v & 31) & np.uint32(1)]

    def next_logits(self):
        """Noise everywhere, the launch's scripted words (and, to show the ban, the stream's banned ids) far above it."""
        n = len(self.cases)
        logits = (self.rs.randn(n, self.V) * 0.5).astype(np.float32)
        for i, h in enumerate(self.hosts):
            if h.wants_draw():
                logits[i, self.cases[i][4][self.launches[i]]] = BOOST
                logits[i, self.ban_of(i)] = BOOST
                self.launches[i] += 1
        if self.guide:                                               # a follower is shown its leader's scripted words
            for r in range(n):
                c = int(self.guide['guide_cond'][r])
                if c >= 0 and c != r:
                    logits[r, logits[c] == BOOST] = BOOST
        return logits

    def drawn_from(self, logits, i):
        """(the row stream i draws from, its column of uniforms): its own, or the host-combined row of its pair and the leader's column."""
        if self.guide and self.guide['guide_cond'][i] >= 0:
            c, g, s = int(self.guide['guide_cond'][i]), int(self.guide['guide_uncond'][i]), np.float32(self.guide['guide_scale'][i])
            return logits[c] + s * (logits[c] - logits[g]), c
        return logits[i], i

    def launch_and_check(self, step):
        from emo_disentanger_amd import ops
        inf = self.inf
        logits = self.next_logits()
        before = {k: self.t[k].cpu().numpy().copy() for k in ('seq', 'segs', 'state')}
        self.logits.copy_(T(logits))
        ops.grammar_step(self.args)
        torch.cuda.synchronize()
        c = self.controls
        for i, h in enumerate(self.hosts):
            row, col = self.drawn_from(logits, i)
            temp = float(c['temp_of'][i]) if c else 1.2
            top_p = float(c['top_p_of'][i]) if c else 0.9
            n0 = len(h.cells)
            h.step(lambda d, i=i: ref_pick(row, self.ban_of(i), temp, top_p, self.U[d, col], self.V), N_U)
            if len(h.cells) > n0:
                self.drawn.append((i, h.cells[-1], h.s.generated[h.cells[-1]], logits[i].copy()))
        st, sq, sg, tk, sk = (self.t[k].cpu().numpy() for k in ('state', 'seq', 'segs', 'tok_out', 'seg_out'))
        for i, h in enumerate(self.hosts):
            for k, v in h.state().items():
                assert st[i, k] == v, (step, i, k, st[i].tolist(), h.state())
            ln = len(h.s.generated)
            assert sq[i, :ln].tolist() == h.s.generated and (sq[i, ln:] == 0).all(), (step, i)
            assert sg[i, :len(h.s.seg)].tolist() == h.s.seg and (sg[i, ln:] == 0).all(), (step, i)
            assert (tk[i], sk[i]) == (h.tok, h.seg), (step, i)
            if h.status == inf.ACC_OVERFLOW and before['state'][i, inf.ACC_S_STATUS] == inf.ACC_RUNNING:
                # the row, LEN, ACCEPTED and DRAWS (and every other word but the status) as they were before the draw
                assert np.array_equal(sq[i], before['seq'][i]) and np.array_equal(sg[i], before['segs'][i]), (step, i)
                assert st[i, 1:].tolist() == before['state'][i, 1:].tolist(), (step, i)
        assert int(self.t['running'].item()) == sum(h.status == inf.ACC_RUNNING for h in self.hosts)

    def run(self):
        step = 0
        while any(h.status == self.inf.ACC_RUNNING for h in self.hosts):
            self.launch_and_check(step)
            step += 1
            assert step < 80
        self.launch_and_check(step)                                  # one launch on finished streams: pad everywhere
        assert (self.t['tok_out'].cpu().numpy() == PAD).all()
        return step


def controls_for(V, n=N):
    """Two ban rows (ids on both sides of a 32-bit word boundary and the last id; id 1, 2 and 32 are also KEPT tokens: fed, banned or not) and
    per-stream temp / top_p."""
    words = (V + 31) // 32
    mask = np.zeros((2, words), np.uint32)
    for m, ids in enumerate(([1, 32, V - 1 if V > 33 else 12], [2, 31 + 1])):
        for v in ids:
            mask[m, v >> 5] |= np.uint32(1 << (v & 31))
    rs = np.random.RandomState(3)
    return dict(tok_mask=mask, mask_of=np.array([0, 0, 1, 0, -1, 1, 1, -1][:n], np.int32),
                temp_of=rs.uniform(0.8, 1.4, n).astype(np.float32), top_p_of=rs.uniform(0.8, 0.97, n).astype(np.float32))


@pytest.mark.parametrize('ctl', [False, True], ids=['plain', 'controls'])
@pytest.mark.parametrize('V', [33, 327])
def test_every_launch_leaves_what_the_host_stream_with_keep_leaves(V, ctl):
    rig = Rig(V, controls=controls_for(V) if ctl else None, seed=V + ctl)
    inf = rig.inf
    rig.run()
    h = rig.hosts
    assert [x.status for x in h] == WANT
    assert rig.launches == [len(c[4]) for c in CASES]                           # every scripted launch was used, nothing more
    assert h[0].s.generated_bars == 3 and h[0].accepted == 4 and h[0].draws == 4
    assert h[1].s.generated_bars == 4 and h[1].accepted == 3                    # two bars were closed by the chain
    assert h[2].s.generated_bars == 3 and h[2].accepted == 3
    assert h[3].s.generated[-3:] == [1, 2, EOS] and h[3].s.generated_bars == 1
    assert h[4].draws == 1 and h[4].accepted == 1 and h[4].s.generated_bars == 0 and len(h[4].s.generated) == opened(0) + 1
    assert len(h[5].s.generated) == opened(1) + 3 and h[5].s.generated[-3:] == [1, 2, 31] and h[5].s.generated_bars == 1
    assert h[6].draws == 4 and h[6].accepted == 3 and h[6].s.failed_cnt == 0
    assert h[7].s.keep is None and h[7].s.generated_bars == 2
    st = rig.t['state'].cpu().numpy()
    assert (st[:, inf.ACC_S_ACCEPTED] == [x.accepted for x in h]).all()


def ref_scores(row, tok):
    l = row.astype(np.float64)
    mx = l.max()
    lse = mx + np.log(np.exp(l - mx).sum())
    p = np.exp(l - lse)
    return l[tok] - lse, int((l > l[tok]).sum() + (l[:tok] == l[tok]).sum()), lse - float((p * l).sum())


def test_the_score_tables_hold_the_accepted_draws_and_nothing_in_kept_cells():
    rig = Rig(327, scores=True, seed=5)
    rig.run()
    lp, rk, en = (rig.tabs[k].cpu().numpy() for k in TABLES)
    cells = np.zeros((N, WIDTH), bool)
    for i, h in enumerate(rig.hosts):
        cells[i, h.cells] = True
    assert cells.sum() == sum(h.accepted for h in rig.hosts) >= 20
    assert np.array_equal(rk >= 0, cells) and np.array_equal(~np.isnan(lp), cells) and np.array_equal(~np.isnan(en), cells)
    for i, c, tok, row in rig.drawn:
        logp, rank, ent = ref_scores(row, tok)
        tol = ROW_TOL * max(1.0, float(np.spacing(np.float32(np.abs(row).max()))) / ULP16)
        assert rk[i, c] == rank and abs(float(lp[i, c]) - logp) <= tol and abs(float(en[i, c]) - ent) <= tol, (i, c)
    # the kept bar of stream 0 lies behind its second accepted draw, the Track_LeadSheet: four tokens without a cell
    h = rig.hosts[0]
    at = h.cells[1]
    assert h.s.generated[at] == TRACK_LS and h.s.generated[at + 5:at + 9] == [1, BEAT(9), BEAT(2), 32] and not cells[0, at + 1:at + 10].any()


def test_with_the_keep_tables_null_the_block_leaves_what_the_launch_without_the_fields_leaves():
    from emo_disentanger_amd import ops
    plain = [(c[0], None, c[2], c[3], c[4] + [[TRACK_LS]] * 4) for c in CASES]
    a, b = Rig(327, cases=plain, keep_tables=False, scores=True, seed=9), Rig(327, cases=plain, keep_tables=False, scores=True, seed=9)
    assert a.args.keep_tok is None and a.args.keep_beg is None and a.args.keep_end is None and a.args.n_keep == 0
    for step in range(24):
        logits = a.next_logits()
        b.launches = list(a.launches)
        a.logits.copy_(T(logits))
        ops.grammar_step(a.args)
        t = b.t                                                                 # a fresh block per call, built by the wrapper that never names the fields
        ops.acc_grammar_step(T(logits), 1.2, 0.9, t['u_steps'], t['ev_flags'], t['ev_beat'], t['lead_tok'], t['lead_off'], t['params'], t['state'],
                             t['seq'], t['segs'], W, TRACK_FULL, PAD, t['tok_out'], t['seg_out'], t['running'], **b.tabs)
        torch.cuda.synchronize()
        for i, h in enumerate(a.hosts):                                         # (the hosts only tell next_logits who draws)
            h.step(lambda d, i=i: ref_pick(logits[i], [], 1.2, 0.9, a.U[d, i], 327), N_U)
        for k in ('tok_out', 'seg_out', 'state', 'seq', 'segs', 'running'):
            assert torch.equal(a.t[k], b.t[k]), (step, k)
    for k in TABLES:
        assert np.array_equal(a.tabs[k].view(torch.int32).cpu().numpy(), b.tabs[k].view(torch.int32).cpu().numpy()), k
    assert int(a.t['running'].item()) == 0


def test_a_guided_pair_with_kept_bars_stays_in_lock_step_with_the_host():
    cases = [CASES[0], CASES[0], CASES[1], CASES[7]]
    guide = dict(guide_cond=np.array([0, 0, -1, -1], np.int32), guide_uncond=np.array([1, 1, -1, -1], np.int32),
                 guide_scale=np.array([1.5, 1.5, 0, 0], np.float32))
    for V in (33, 327):
        rig = Rig(V, cases=cases, guide=guide, seed=V)
        rig.run()
        a, b = rig.hosts[0], rig.hosts[1]
        assert a.status == b.status == 1 and a.s.generated == b.s.generated and a.s.generated_bars == 3 and a.accepted == b.accepted == 4
        sq = rig.t['seq'].cpu().numpy()
        assert np.array_equal(sq[0], sq[1]) and rig.hosts[2].status == 1 and rig.hosts[3].status == 1


def test_the_block_setter_checks_the_keep_tables():
    from emo_disentanger_amd import ops
    rig = Rig(33)
    n_off = rig.t['lead_off'].numel()
    good = {k: rig.held[k] for k in ('keep_tok', 'keep_beg', 'keep_end')}
    for bad, what in ((dict(good, keep_end=None), 'come together'), (dict(good, keep_beg=good['keep_beg'][:n_off - 1].contiguous()), 'one entry per entry of lead_off'),
                      (dict(good, keep_beg=good['keep_beg'].long()), 'bad dtype / layout of keep_beg'),
                      (dict(good, keep_tok=good['keep_tok'].int()), 'bad dtype / layout of keep_tok'),
                      (dict(good, keep_end=good['keep_end'] + 1000), 'outside keep_tok')):
        args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
        with pytest.raises(AssertionError, match=what):
            ops.block_set(args, held, logits=rig.logits, **rig.num, **rig.t, **bad)
        if 'layout of' in what:                                     # the refused tensor never enters the block (the launch refuses the other two alone)
            assert getattr(args, what.split()[-1]) is None and what.split()[-1] not in held
        else:                                                       # a set that fails the joint check leaves the block as a whole
            assert args.keep_tok is None and args.keep_beg is None and args.keep_end is None


# ------------------------------------------------------------------------------------------------ kind ACC_QUEUE
def test_a_queued_job_admitted_mid_run_whose_first_two_bars_are_kept():
    """Two slots, three jobs: jobs 0 and 1 are short and end in different launches; job 2, admitted into the slot that frees first, has its first
    two bars kept (in its row at load, fed token by token from position 0), draws bar 2 and gets bar 3 from the chain in the launch."""
    from emo_disentanger_amd import inference as inf, ops
    V = 33
    e2i, i2e = vocab(V)
    jobs = [(1, None, [[31], [TRACK_LS]]), (1, None, [[30], [29], [TRACK_LS]]), (5, [[1, 2], [], None, [31, BEAT(3)], None], [[29], [TRACK_LS], [TRACK_LS]])]
    n, slots = len(jobs), 2
    leads = [LEAD[:j[0]] for j in jobs]
    keeps = [j[1] for j in jobs]
    hosts = [Host(inf, e2i, i2e, leads[i], PRIMER, keeps[i], 1000, 1) for i in range(n)]
    assert hosts[2].s.generated_bars == 2 and hosts[2].s.generated == PRIMER + [TRACK_LS] + LEAD[0] + [TRACK_FULL, 1, 2, TRACK_LS] + LEAD[1] + \
        [TRACK_FULL, TRACK_LS] + LEAD[2] + [TRACK_FULL]
    U = np.full((N_U, n), 0.2, np.float32)
    flags, beat = inf.acc_event_tables(i2e, V)
    toks, offs, bar0, nbars, _ = inf.pack_lead_sheets(leads)
    kt, kb, ke = inf.pack_keep(keeps, leads)
    seq, segs = np.zeros((n, WIDTH), np.int64), np.zeros((n, WIDTH), np.int64)
    params, state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
    for i, h in enumerate(hosts):
        k = len(h.s.generated)
        seq[i, :k], segs[i, :k] = h.s.generated, h.s.seg
        params[i, :5] = h.s.target_bars, 1000, 0, bar0[i], nbars[i]
        state[i, [inf.ACC_S_STATUS, inf.ACC_S_LEN, inf.ACC_S_CONSUMED, inf.ACC_S_BARS]] = inf.ACC_RUNNING, k, 1, h.s.generated_bars
    t = dict(u_steps=T(U), ev_flags=T(flags), ev_beat=T(beat), params=T(params), state=T(state), seq=T(seq), segs=T(segs), lead_tok=T(toks),
             lead_off=T(offs), keep_tok=T(kt), keep_beg=T(kb), keep_end=T(ke), tok_out=torch.full((slots,), PAD, dtype=torch.long, device=DEV),
             seg_out=torch.ones(slots, dtype=torch.long, device=DEV), running=torch.tensor([n], dtype=torch.int32, device=DEV),
             slot_job=torch.full((slots,), -1, dtype=torch.int32, device=DEV), queue_head=torch.zeros(1, dtype=torch.int32, device=DEV),
             mem_lens=torch.zeros(slots, dtype=torch.long, device=DEV), row_reset=torch.zeros(slots, dtype=torch.int32, device=DEV),
             job_steps=torch.full((n,), -7, dtype=torch.int32, device=DEV))
    logits_d = torch.zeros(slots, V, device=DEV)
    args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC_QUEUE), {}
    ops.block_set(args, held, n_rows=slots, n_token=V, ld_u=n, temperature=1.2, top_p=0.9, track_full=TRACK_FULL, max_len=W, pad=PAD, n_jobs=n,
                  mem_rows=W, n_keep=4, keep_eos=EOS, logits=logits_d, **t)
    held_by, launches, admitted_at = [-1] * slots, [0] * n, {}
    for step in range(60):
        logits = np.zeros((slots, V), np.float32)
        for b, j in enumerate(held_by):
            if j >= 0 and hosts[j].wants_draw():
                logits[b, jobs[j][2][launches[j]]] = BOOST
                launches[j] += 1
        logits_d.copy_(T(logits))
        ops.grammar_step(args)
        torch.cuda.synchronize()
        now = t['slot_job'].cpu().tolist()
        tk, sk, ml, rr = (t[k].cpu().tolist() for k in ('tok_out', 'seg_out', 'mem_lens', 'row_reset'))
        for b, j in enumerate(held_by):
            if j >= 0:
                hosts[j].step(lambda d, b=b, j=j: ref_pick(logits[b], [], 1.2, 0.9, U[d, j], V), N_U)
            if j >= 0 and hosts[j].status == inf.ACC_RUNNING:
                assert now[b] == j and (tk[b], sk[b], ml[b], rr[b]) == (hosts[j].tok, hosts[j].seg, hosts[j].s.consumed - 1, 0), (step, b)
            elif now[b] >= 0:                                       # the slot admitted a job in this launch: its first token, position 0
                j2 = now[b]
                assert j2 not in admitted_at and hosts[j2].s.consumed == 1
                admitted_at[j2] = step
                assert (tk[b], sk[b], ml[b], rr[b]) == (hosts[j2].s.generated[0], hosts[j2].s.seg[0], 0, 1), (step, b)
            else:
                assert (tk[b], sk[b], ml[b], rr[b]) == (PAD, 1, 0, 0), (step, b)
        held_by = now
        st, sq, sg = (t[k].cpu().numpy() for k in ('state', 'seq', 'segs'))
        for i, h in enumerate(hosts):
            if i in admitted_at:
                for k, v in h.state().items():
                    assert st[i, k] == v, (step, i, k, st[i].tolist(), h.state())
            assert sq[i, :len(h.s.generated)].tolist() == h.s.generated and sg[i, :len(h.s.seg)].tolist() == h.s.seg, (step, i)
        if all(h.status != inf.ACC_RUNNING for h in hosts):
            break
    assert [h.status for h in hosts] == [1, 1, 1] and int(t['running'].item()) == 0
    assert admitted_at[0] == admitted_at[1] == 0 and admitted_at[2] > 0 and launches == [2, 3, 3]
    h = hosts[2]
    assert h.s.generated_bars == 5 and h.accepted == 3 and h.draws == 3
    # bar 3 came from the chain behind the Track_LeadSheet that closed bar 2; bar 4, the last, was drawn and closed by the last Track_LeadSheet
    tail = [TRACK_LS] + LEAD[3] + [TRACK_FULL, 31, BEAT(3), TRACK_LS] + LEAD[4] + [TRACK_FULL, TRACK_LS]
    assert h.s.generated[-len(tail):] == tail
    assert t['job_steps'].cpu().tolist() == [x.s.consumed for x in hosts]        # the tokens each job was fed
