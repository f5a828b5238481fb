"""GPU: stage-2 generation from a queue (emo_grammar_step, kind ACC_QUEUE; emo_favor_state_reset; inference.AccompanimentQueue).  The kernel
against the host grammar (_Stream.offer) launch by launch with no model, admissions checked after every launch; its scores; the reset kernel;
what a slot's logits are (each job against a one-row engine of its own); the window; the one-launch step under graph replay; and
generate_accompaniments(slots=) end to end.
Bounds: fp32 logits of two routes to the same value within LOGIT_TOL x the logits' scale (tests/test_gpu_stage1_queue.py); the one-launch step
against a second engine within 2 % of the logit range (the same file, one-launch bf16); recorded figures at row_tol of tests/test_gpu_draw_scores.py
(ROW_TOL there); ids drawn with ops.sample_nucleus are exact."""
import copy
import functools

import numpy as np
import pytest
import torch

from test_gpu_draw_scores import ref_scores, row_tol
from test_gpu_stage2_window import _host_window_loop, _tiny, _vocab

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
DEV = 'cuda'


# ------------------------------------------------------------------------------------------------ the kernel, launch by launch
class HostJob:
    """One job of the queue restated on _Stream.offer: what acc_stream_step does to it in one launch."""

    def __init__(self, inf, e2i, i2e, lead, primer, max_bars, max_events, skip_check):
        self.inf, self.e2i, self.i2e = inf, e2i, i2e
        self.s = inf._Stream(e2i, lead, primer, max_bars)
        self.max_events, self.skip = max_events, skip_check
        self.status = inf.ACC_DONE if self.s.done else inf.ACC_RUNNING
        self.draws = self.accepted = 0
        self.consumed = 1                                   # (what an admission sets; the tables are built with it)
        self.cell = None                                    # (column, token) of the draw accepted in the last launch

    def feed(self):
        s = self.s
        tok, seg = s.generated[self.consumed], s.seg[self.consumed]
        self.consumed += 1
        return tok, seg

    def offer(self, w, n_u):
        """One draw through the grammar -> True when the launch draws again."""
        inf, s = self.inf, self.s
        self.draws += 1
        before = len(s.generated)
        ok = s.offer(w, self.e2i, self.i2e, self.skip, self.max_events)
        if s.stuck:
            self.status = inf.ACC_STUCK
        elif ok:
            self.accepted += 1
            self.cell = (before, w)
            if s.done:
                self.status = inf.ACC_DONE
        elif self.draws >= n_u:
            self.status = inf.ACC_OUT_OF_DRAWS
        else:
            return True
        return False

    def state(self):
        inf, s = self.inf, self.s
        return {inf.ACC_S_STATUS: self.status, inf.ACC_S_LEN: len(s.generated), inf.ACC_S_CONSUMED: self.consumed, inf.ACC_S_BARS: s.generated_bars,
                inf.ACC_S_CUR_POS: s.cur_pos, inf.ACC_S_FAILED: s.failed_cnt, inf.ACC_S_DRAWS: self.draws, inf.ACC_S_ACCEPTED: self.accepted}


# lead sheet (bar indices into generate.json's lead), primer, max_bars, max_events, skip_check.  max_bars 0: closed on the host before the run.
JOBS11 = [
    ([0, 1, 2], [0, 4, 6], None, 60, False), ([0, 1], [1, 5, 6], None, 60, False), ([2], [2, 4, 6], None, 40, False),
    ([0, 1, 2, 0], [3, 5, 6], 0, 60, False),                                                      # closed
    ([1, 0], [0, 5, 6], None, 60, True), ([2, 1, 0], [1, 4, 6], None, 22, False), ([0], [2, 5, 6], None, 60, False),
    ([1, 2], [3, 4, 6], None, 60, False), ([0, 1, 2, 0, 1], [0, 4, 6], None, 200, False), ([2, 2], [1, 5], None, 60, False),
    ([1], [2, 4, 6, 26, 27], None, 60, False),
]
W_Q, WIDTH_Q, NU_Q, SLOTS_Q = 40, 56, 400, 3


class KernelRig:
    """The queue kernel and its host restatement side by side, no model: fresh seeded random logits [slots, V] per launch, each row at a scale
    of its own (flat rows: PAD, early EOS and Beats below the position get drawn and redrawn; peaked rows: one word again and again, which is
    how 256 rejected Beats in a row — STUCK — come about)."""

    def __init__(self, scores=True, seed=14):
        from emo_disentanger_amd import inference as inf, ops
        self.inf, self.ops = inf, ops
        g, e2i, i2e = _vocab()
        self.e2i, self.V, n = e2i, len(i2e), len(JOBS11)
        leads = [[list(g['lead'][k]) for k in j[0]] for j in JOBS11]
        self.hosts = [HostJob(inf, e2i, i2e, ld, j[1], j[2], j[3], j[4]) for j, ld in zip(JOBS11, leads)]
        flags, beat = inf.acc_event_tables(i2e, self.V)
        toks, offs, bar0, nbars, longest = inf.pack_lead_sheets(leads)
        assert WIDTH_Q >= W_Q + longest + 2
        seq, segs = np.zeros((n, WIDTH_Q), np.int64), np.zeros((n, WIDTH_Q), np.int64)
        params, state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
        for i, (h, j) in enumerate(zip(self.hosts, JOBS11)):
            k = len(h.s.generated)
            seq[i, :k], segs[i, :k] = h.s.generated, h.s.seg
            params[i, :5] = h.s.target_bars, j[3], j[4], bar0[i], nbars[i]
            for w, v in h.state().items():
                state[i, w] = v
            state[i, inf.ACC_S_CONSUMED] = 23                       # (whatever the host leaves there is ignored: an admission sets 1)
        T = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
        self.t = dict(seq=T(seq), segs=T(segs), state=T(state), tok_out=torch.full((SLOTS_Q,), -5, dtype=torch.long, device=DEV),
                      seg_out=torch.full((SLOTS_Q,), -5, dtype=torch.long, device=DEV), running=torch.tensor([self.live()], dtype=torch.int32, device=DEV),
                      slot_job=torch.full((SLOTS_Q,), -1, dtype=torch.int32, device=DEV), queue_head=torch.zeros(1, dtype=torch.int32, device=DEV),
                      mem_lens=torch.full((SLOTS_Q,), 9, dtype=torch.long, device=DEV), row_reset=torch.full((SLOTS_Q,), 7, dtype=torch.int32, device=DEV),
                      job_steps=torch.full((n,), -7, dtype=torch.int32, device=DEV))
        self.fixed = dict(ev_flags=T(flags), ev_beat=T(beat), lead_tok=T(toks), lead_off=T(offs), params=T(params))
        self.Uh = np.random.RandomState(seed + 100).uniform(size=(NU_Q, n)).astype(np.float32)
        self.U = T(self.Uh)
        self.tabs = ops.draw_score_tables(self.t['seq']) if scores else {}
        self.tabs0 = {k: v.clone() for k, v in self.tabs.items()}
        self.rs = np.random.RandomState(seed)
        self.book = [-1] * SLOTS_Q
        self.open = [j for j, h in enumerate(self.hosts) if h.status == inf.ACC_RUNNING]
        self.head, self.admitted, self.steps, self.launches, self.drained = 0, [], {}, 0, None
        self.cells, self.seen = {}, dict(rejected=0, redraw_launches=0, refilled=0)
        self.history, self.twins = [], 0                    # per launch: every tensor the launch may write

    def live(self):
        return sum(h.status == self.inf.ACC_RUNNING for h in self.hosts)

    def launch(self):
        inf, ops, t, pad = self.inf, self.ops, self.t, self.e2i['PAD_None']
        logits = (self.rs.randn(SLOTS_Q, self.V) * self.rs.choice([1.5, 4.0, 40.0], size=(SLOTS_Q, 1), p=[0.45, 0.35, 0.2])).astype(np.float32)
        lg = torch.from_numpy(logits).to(DEV)
        twin = {k: v.clone() for k, v in t.items()} if self.tabs else None
        ops.acc_queue_step(lg, 1.2, 0.9, self.U, self.fixed['ev_flags'], self.fixed['ev_beat'], self.fixed['lead_tok'], self.fixed['lead_off'],
                           self.fixed['params'], t['state'], t['seq'], t['segs'], W_Q, self.e2i['Track_Full'], pad, t['tok_out'], t['seg_out'],
                           t['running'], t['slot_job'], t['queue_head'], t['mem_lens'], W_Q, t['row_reset'], job_steps=t['job_steps'], **self.tabs)
        self.launches += 1
        where = self.launches
        if twin is not None:
            # the same launch on a copy of everything it may write, with the three score pointers NULL: bit-equal.  (Which of several slots that
            # free up in one launch gets which job is the device's choice in each launch, so the slot arrays are compared slot by slot where the
            # two launches gave the slot the same job, and as a whole after sorting.)
            ops.acc_queue_step(lg, 1.2, 0.9, self.U, self.fixed['ev_flags'], self.fixed['ev_beat'], self.fixed['lead_tok'], self.fixed['lead_off'],
                               self.fixed['params'], twin['state'], twin['seq'], twin['segs'], W_Q, self.e2i['Track_Full'], pad, twin['tok_out'],
                               twin['seg_out'], twin['running'], twin['slot_job'], twin['queue_head'], twin['mem_lens'], W_Q, twin['row_reset'],
                               job_steps=twin['job_steps'])
            for k in ('state', 'seq', 'segs', 'running', 'job_steps'):
                assert torch.equal(t[k], twin[k]), (where, k)
            per_slot = [list(zip(*(x[k].cpu().tolist() for k in ('slot_job', 'tok_out', 'seg_out', 'mem_lens', 'row_reset')))) for x in (t, twin)]
            assert sorted(per_slot[0]) == sorted(per_slot[1]), (where, per_slot)
            assert all(a == b for a, b in zip(*per_slot) if a[0] == b[0]), (where, per_slot)
            self.twins += 1
        # the restatement: every slot that holds a RUNNING job
        expect, want = {}, []
        for b, j in enumerate(self.book):
            if j < 0:
                continue
            h = self.hosts[j]
            h.cell = None
            assert h.status == inf.ACC_RUNNING
            if len(h.s.generated) >= W_Q:
                h.status = inf.ACC_WINDOW
            elif h.consumed < len(h.s.generated):
                expect[b] = h.feed()
            else:
                want.append(b)
        drew, first = list(want), True
        while want:                                   # one draw for every slot that wants one, again for the rejected ones
            u = torch.zeros(SLOTS_Q, device=DEV)
            for b in want:
                u[b] = float(self.Uh[min(self.hosts[self.book[b]].draws, NU_Q - 1), self.book[b]])       # draw d of JOB j: row d, column j
            words = ops.sample_nucleus(lg, 1.2, 0.9, u).cpu().tolist()
            want = [b for b in want if self.hosts[self.book[b]].offer(words[b], NU_Q)]
            self.seen['rejected'] += len(want)
            self.seen['redraw_launches'] += bool(want) and first
            first = False
        for b in drew:
            h = self.hosts[self.book[b]]
            assert len(h.s.generated) <= WIDTH_Q
            if h.cell is not None:
                self.cells[(self.book[b], h.cell[0])] = (logits[b], h.cell[1])
            if h.status == inf.ACC_RUNNING:
                expect[b] = h.feed()
        st, sq, sg = t['state'].cpu().numpy(), t['seq'].cpu().numpy(), t['segs'].cpu().numpy()
        tk, sv, sj = t['tok_out'].cpu().tolist(), t['seg_out'].cpu().tolist(), t['slot_job'].cpu().tolist()
        ln, rr = t['mem_lens'].cpu().tolist(), t['row_reset'].cpu().tolist()
        freed = []
        for b, j in enumerate(self.book):
            if j < 0:
                freed.append(b)
                continue
            h = self.hosts[j]
            for k, v in h.state().items():              # every state word of the job
                assert st[j, k] == v, (where, b, j, k, st[j].tolist(), h.state())
            assert sq[j, :len(h.s.generated)].tolist() == h.s.generated and sg[j, :len(h.s.seg)].tolist() == h.s.seg, (where, b, j)
            if h.status == inf.ACC_RUNNING:
                assert sj[b] == j and (tk[b], sv[b]) == expect[b] and ln[b] == h.consumed - 1 and rr[b] == 0, (where, b, j, tk, sv, ln, rr)
            else:
                self.steps[j] = h.consumed
                self.seen['refilled'] += sj[b] >= 0
                freed.append(b)
        # admissions: the freed slots hold the next consecutive open jobs from the head (which slot got which is the device's choice)
        nxt = self.open[self.head:self.head + len(freed)]
        got = sorted(sj[b] for b in freed if sj[b] >= 0)
        assert got == nxt, (where, freed, sj, self.head)
        for b in freed:
            self.book[b] = sj[b]
            assert ln[b] == 0 and rr[b] == (1 if sj[b] >= 0 else 0), (where, b, ln, rr)
            if sj[b] >= 0:
                h = self.hosts[sj[b]]
                assert (tk[b], sv[b]) == (h.s.generated[0], h.s.seg[0]) and st[sj[b], inf.ACC_S_CONSUMED] == 1, (where, b)
            else:
                assert (tk[b], sv[b]) == (pad, 1), (where, b)
        self.head += len(nxt)
        self.admitted += nxt
        # queue_head: every popped index lies in front of the last admitted job (a slot that pops a closed job pops again), so while every freed
        # slot got a job it is exactly that job's index + 1; once a slot found the queue empty it is at least n and at most n + slots
        qh, n = int(t['queue_head'].item()), len(self.hosts)
        if freed and len(nxt) == len(freed):
            assert qh == nxt[-1] + 1, (where, qh, nxt)
        elif freed:
            assert n <= qh <= n + SLOTS_Q, (where, qh)
        assert int(t['running'].item()) == self.live(), where
        self.history.append({k: v.cpu().numpy().copy() for k, v in t.items() if k != 'queue_head'})

    def run(self, limit=900):
        self.launch()                                     # the first launch admits, nothing else
        assert self.admitted == self.open[:SLOTS_Q]
        while self.live() > 0:
            self.launch()
            assert self.launches < limit
        self.drained = self.launches
        return self


@functools.lru_cache(None)
def _stepped():
    return KernelRig().run()


def test_queue_kernel_matches_the_host_grammar_and_admits_in_order():
    rig = _stepped()
    inf = rig.inf
    status = [h.status for h in rig.hosts]
    # the chosen seed produces each of these at least once (counted by the restatement, which is _Stream.offer on the host)
    eos = rig.e2i['EOS_None']
    print('[measured] 11 jobs / 3 slots: %d launches, endings %s, %r' % (rig.drained, status, rig.seen))
    assert rig.seen['rejected'] >= 5 and rig.seen['redraw_launches'] >= 3 and rig.seen['refilled'] >= 3
    assert inf.ACC_STUCK in status and inf.ACC_DONE in status
    assert any(h.status == inf.ACC_DONE and h.s.generated[-1] == eos for h in rig.hosts)
    assert rig.open == [0, 1, 2, 4, 5, 6, 7, 8, 9, 10] and rig.admitted == rig.open                  # the closed job is passed over
    st = rig.t['state'].cpu().numpy()
    assert st[3, inf.ACC_S_DRAWS] == 0 and st[3, inf.ACC_S_CONSUMED] == 23 and int(rig.t['job_steps'][3]) == -7
    # after the drain: every slot free at position 0 with pad, and it stays so
    assert rig.book == [-1] * SLOTS_Q
    head = int(rig.t['queue_head'].item())
    last = rig.history[-1]
    for _ in range(3):
        rig.launch()
        for k, v in rig.history[-1].items():
            assert np.array_equal(v, last[k]), k
    assert int(rig.t['queue_head'].item()) == head and rig.t['mem_lens'].tolist() == [0] * SLOTS_Q
    assert rig.t['tok_out'].tolist() == [rig.e2i['PAD_None']] * SLOTS_Q and rig.t['slot_job'].tolist() == [-1] * SLOTS_Q
    # the launches a job held its slot, as the kernel wrote them, and the plan they give
    from emo_disentanger_amd.stage1_inference import queue_plan
    steps = rig.t['job_steps'].tolist()
    assert [steps[j] for j in rig.open] == [rig.steps[j] for j in rig.open]
    assert queue_plan([steps[j] for j in rig.open], SLOTS_Q)[0] == rig.drained


def test_queue_kernel_scores_exactly_the_accepted_draws_and_changes_nothing_else():
    with_t = _stepped()
    assert with_t.twins >= with_t.drained                               # every launch also ran with NULL score pointers: everything else bit-equal
    tabs = {k: v.cpu().numpy() for k, v in with_t.tabs.items()}
    written = np.zeros(tabs['tok_rank'].shape, bool)
    worst = 0.0
    assert len(with_t.cells) == sum(h.accepted for h in with_t.hosts) >= 40
    for (j, c), (row, tok) in with_t.cells.items():
        written[j, c] = True
        logp, rank, ent = ref_scores(row, tok)
        e = max(abs(float(tabs['tok_logp'][j, c]) - logp), abs(float(tabs['tok_entropy'][j, c]) - ent)) / row_tol(row)
        worst = max(worst, e)
        assert tabs['tok_rank'][j, c] == rank, (j, c)
    print('[measured] recorded logp / entropy against float64 on the slot\'s row: worst %.3f of row_tol over %d cells' % (worst, len(with_t.cells)))
    assert worst <= 1.0
    for k, v in with_t.tabs.items():                                    # every other cell holds what the caller put there
        same = (v.view(torch.int32) == with_t.tabs0[k].view(torch.int32)).cpu().numpy()
        assert np.array_equal(~same, written), k


# ------------------------------------------------------------------------------------------------ the reset kernel
def test_state_reset_zeroes_the_flagged_rows_and_touches_no_other():
    from emo_disentanger_amd import ops
    L, n, H, F, dh = 3, 5, 4, 32, 16                                    # S row 2048 floats, z row 128: one chunk holds the end of S and all of z
    gen = torch.Generator(device=DEV).manual_seed(1)
    S = [torch.randn(n, H, F, dh, device=DEV, generator=gen) + 3.0 for _ in range(L)]
    z = [torch.randn(n, H, F, device=DEV, generator=gen) + 3.0 for _ in range(L)]
    table = torch.tensor([[S[l].data_ptr(), z[l].data_ptr()] for l in range(L)], dtype=torch.int64, device=DEV)
    S0, z0 = [x.clone() for x in S], [x.clone() for x in z]
    flags = torch.zeros(n, dtype=torch.int32, device=DEV)
    ops.favor_state_reset(table, n, H * F * dh, H * F, flags)
    for l in range(L):                                                  # all-zero flags change nothing
        assert torch.equal(S[l], S0[l]) and torch.equal(z[l], z0[l])
    flags.copy_(torch.tensor([0, 1, 0, 1, 0], dtype=torch.int32))
    ops.favor_state_reset(table, n, H * F * dh, H * F, flags)
    for l in range(L):
        for r in range(n):
            if r in (1, 3):
                assert not S[l][r].any() and not z[l][r].any(), (l, r)
            else:
                assert torch.equal(S[l][r], S0[l][r]) and torch.equal(z[l][r], z0[l][r]), (l, r)
    # a row longer than one chunk (S row 8192 floats = 2 chunks, z in a third)
    S2, z2 = torch.ones(2, 8, 64, 16, device=DEV), torch.ones(2, 8, 64, device=DEV)
    t2 = torch.tensor([[S2.data_ptr(), z2.data_ptr()]], dtype=torch.int64, device=DEV)
    ops.favor_state_reset(t2, 2, 8192, 512, torch.tensor([1, 0], dtype=torch.int32, device=DEV))
    assert not S2[0].any() and not z2[0].any() and bool((S2[1] == 1).all()) and bool((z2[1] == 1).all())


# ------------------------------------------------------------------------------------------------ every job against an engine of its own
def _jobs(g, n):
    lead = [list(b) for b in g['lead']]
    leads = [lead * 2, lead[:1], lead[::-1], [lead[1]] * 3, lead, lead[1:], lead * 3, lead[:2], lead[2:], lead[::-1] * 2]
    primers = [list(g['primer']), [1, 5, 6], [2, 4, 6], [2, 4], [3, 5, 6], [0, 4, 6, 26, 27], [1, 4, 6], [3, 4], [0, 5, 6], [2, 5, 6]]
    return leads[:n], primers[:n]


def _own_engine(inf, model, W):
    if model.kind == 'performer':
        eng = inf.PerformerDecodeEngine(model, 1, redraw=False, persistent=False)
        eng.start_empty()
        return eng
    return inf.GPT2DecodeEngine(model, 1, max_len=W, persistent=False)


@pytest.mark.parametrize('kind', ['gpt2', 'performer'])
def test_a_slots_logits_are_those_of_an_engine_of_the_jobs_own(kind, monkeypatch):
    # The queue loop stepped by hand on the chain of launches in fp32, 10 jobs through 3 slots.  Beside it runs a ONE-ROW engine per job, created
    # when the job is admitted and fed, by plain step() calls (host positions 0, 1, 2, ...), exactly the token and segment its slot was fed in
    # every launch; the position the slot was fed at is checked against that count.  At every draw the slot's logits row is held to the job's
    # own row; the accepted id is drawn again from the job's own row wherever the two rows are bit-equal.  The first step of a job in a row
    # that held another job before (a restarted row) is also held to a one-token prefill.
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 64)
    model = _tiny(kind, 'fp32', tls_bias=3.0)
    leads, primers = _jobs(g, 10)
    q = inf.AccompanimentQueue(model, e2i, i2e, leads, primers, 3, max_events=60, temp=1.2, top_p=0.95, seed=11, redraw=False, scores=True)
    assert q.eng.persist is None and (q.state_table is not None) == (kind == 'performer')
    n = q.n
    own_eng, own, used = [None] * n, [None] * n, [0] * 3
    err, err0, scale, draws, exact, ids_equal, restarts, launches = 0.0, 0.0, 0.0, 0, 0, 0, 0, 0
    with torch.no_grad():
        while q._live() > 0:
            before, held = q.state.cpu().numpy().copy(), q.slot_job.cpu().tolist()
            slot_logits = q.logits.clone()
            q.grammar()
            launches += 1
            after, seq, now = q.state.cpu().numpy(), q.seq.cpu().numpy(), q.slot_job.cpu().tolist()
            fed, fseg, fpos = q.tok.cpu().tolist(), q.segv.cpu().tolist(), q.eng.pos_dev.cpu().tolist()
            for b, j in enumerate(held):
                if j < 0 or after[j, inf.ACC_S_DRAWS] == before[j, inf.ACC_S_DRAWS]:
                    continue
                d = float((slot_logits[b] - own[j]).abs().max())
                err, scale, draws = max(err, d), max(scale, float(own[j].abs().max())), draws + 1
                if d == 0.0 and after[j, inf.ACC_S_ACCEPTED] != before[j, inf.ACC_S_ACCEPTED]:
                    exact += 1
                    u = q.U[int(after[j, inf.ACC_S_DRAWS]) - 1, j].reshape(1)         # the accepted draw is the launch's last
                    w = ops.sample_nucleus(own[j].view(1, -1).contiguous(), 1.2, 0.95, u)
                    ids_equal += int(w.item()) == int(seq[j, int(before[j, inf.ACC_S_LEN])])
            if q._live() == 0:
                break
            q.model_step()
            for b, j in enumerate(now):
                if j < 0:
                    continue
                if held[b] != j:                                          # admitted in this launch: an engine of its own, from nothing
                    assert own_eng[j] is None and fed[b] == seq[j, 0] and fpos[b] == 0
                    own_eng[j] = _own_engine(inf, model, 64)
                    if used[b]:                                           # the row held another job: its first step against a one-token prefill
                        pre = _own_engine(inf, model, 64).prefill(torch.tensor([[fed[b]]], device=DEV), torch.tensor([[fseg[b]]], device=DEV))
                        err0, restarts = max(err0, float((q.logits[b] - pre[0].float()).abs().max())), restarts + 1
                    used[b] += 1
                assert fpos[b] == own_eng[j].pos, (launches, b, j)
                own[j] = own_eng[j].step(torch.tensor([fed[b]], device=DEV), torch.tensor([fseg[b]], device=DEV)).float().clone()[0]
            assert launches < 1500
    st = q.state.cpu().numpy()
    assert (st[:, inf.ACC_S_STATUS] != inf.ACC_RUNNING).all() and all(e is not None for e in own_eng)
    assert [e.pos for e in own_eng] == q.job_steps()                       # each engine was fed as many tokens as the kernel counted
    print('[measured] %s fp32 chain, 10 jobs / 3 slots, each job against an engine of its own: max |slot - own| = %.3e over %d draws (scale %.3e; '
          'expected 0), bit-equal rows at %d accepted draws, ids equal at %d of them; %d restarted rows against a one-token prefill: %.3e'
          % (kind, err, draws, scale, exact, ids_equal, restarts, err0))
    assert draws >= 40 and restarts >= 5
    assert err <= LOGIT_TOL * scale and err0 <= LOGIT_TOL * scale
    assert ids_equal == exact


# ------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_a_job_at_the_window_frees_its_slot_and_is_finished_as_in_the_lock_step_loop(kind, monkeypatch):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    model = _tiny(kind, 'fp32')
    lead = [list(b) for b in g['lead']]
    leads = [lead * 4, lead[:1], lead[::-1] * 3, [lead[1]] * 9, lead[:2], lead * 3, lead[1:], lead * 2 + lead[:1]]
    primers = [list(g['primer']), [1, 5, 6], [2, 4, 6], [2, 4], [3, 5, 6], [0, 4, 6, 26, 27], [1, 4, 6], [0, 5, 6]]
    kw = dict(max_events=160, skip_check=False, temp=1.2, top_p=0.97, seed=5)
    q = inf.AccompanimentQueue(model, e2i, i2e, leads, primers, 3, redraw=False, **kw)
    refilled = 0
    with torch.no_grad():
        while q._live() > 0:
            held, before = q.slot_job.cpu().tolist(), q.state[:, inf.ACC_S_STATUS].cpu().tolist()
            head = int(q.queue_head.item())
            q.grammar()
            now, after, rr = q.slot_job.cpu().tolist(), q.state[:, inf.ACC_S_STATUS].cpu().tolist(), q.row_reset.cpu().tolist()
            freed = [b for b, j in enumerate(held) if j < 0 or after[j] != inf.ACC_RUNNING]
            assert sum(now[b] >= 0 for b in freed) == min(len(freed), max(0, q.n - head))      # (no job of this queue is closed before the run)
            for b, j in enumerate(held):
                if j >= 0 and before[j] == inf.ACC_RUNNING and after[j] == inf.ACC_WINDOW:
                    assert int(q.state[j, inf.ACC_S_LEN]) >= 48 and now[b] != j
                    if q.n - head >= len(freed) > 0:                      # a job waited for every freed slot: this one took one in the same launch
                        assert now[b] >= 0 and rr[b] == 1 and int(q.eng.pos_dev[b]) == 0
                        refilled += 1
            q.model_step()
    crossed = [i for i in range(q.n) if int(q.state[i, inf.ACC_S_STATUS]) == inf.ACC_WINDOW]
    assert len(crossed) >= 2 and refilled >= 1
    # window='device': the WINDOW jobs together on a WindowedLoop, against the host grammar on the same draws (the lock-step test's restatement)
    wl = inf.WindowedLoop(q, 5)
    assert wl.idx == crossed
    st, status, _ = _host_window_loop(inf, model, e2i, i2e, q, wl, 160, False)
    dev_out = q.results(e2i, i2e, 160, False, 5, window='device')
    for j, i in enumerate(crossed):
        assert dev_out[i] == st[j].result() and len(dev_out[i]) >= 48, i
    # window='host': _resume_windowed on the job rebuilt from the device rows, with the draws of (seed, job)
    handed = {i: copy.deepcopy(q.handed_off(i)) for i in crossed}
    host_out = q.results(e2i, i2e, 160, False, 5, window='host')
    for i in crossed:
        rs = np.random.RandomState([5, i])
        want = inf._resume_windowed(model, e2i, i2e, handed[i], 160, False, 1.2, None, lambda probs, rs=rs: inf.nucleus(probs, 0.97, rng=rs))
        assert host_out[i] == want and host_out[i][:48] == dev_out[i][:48], i
    for i in range(q.n):
        if i not in crossed:
            assert host_out[i] == dev_out[i] and isinstance(host_out[i], list)
    # the public call under graph replay gives the same pieces
    pub, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, slots=3, window='device', **kw)
    same = [a == b for a, b in zip(pub, dev_out)]
    print('[measured] %s: %d of 8 jobs reached the window of 48; generate_accompaniments(slots=3) under replay equals the hand-stepped loop on %d of 8'
          % (kind, len(crossed), sum(same)))
    assert all(same)


# ------------------------------------------------------------------------------------------------ the one-launch step
@functools.lru_cache(None)
def _wide(kind):
    """d 512 / 8 heads / 2 layers / bf16 on the generate.json vocabulary: the shape the one-launch step is built for."""
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    g, e2i, _ = _vocab()
    V = len(e2i)
    torch.manual_seed(5)
    if kind == 'performer':
        m = MusicPerformer(V, 2, 8, 512, 2048, 512, favor_feature_dims=128, use_segment_emb=True, n_segment_types=2, compute_dtype='bf16', redraw='fixed')
    else:
        m = MusicGPT2(V, 2, 8, 512, 2048, 512, use_segment_emb=True, n_segment_types=2, dropout=0.1, compute_dtype='bf16')
    with torch.no_grad():
        m.dec_out_proj.bias[e2i['Track_LeadSheet']] += 2.0              # bars end, pieces finish
    return m.cuda().eval()


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_one_launch_step_under_graph_replay(kind, monkeypatch):
    from emo_disentanger_amd import inference as inf, ops
    if ops.lib.emo_decode_step_supported() != 1:
        pytest.skip('the one-launch decode step needs the whole device (emo_decode_step_supported)')
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 64)
    model = _wide(kind)
    leads, primers = _jobs(g, 9)
    kw = dict(max_events=60, temp=1.2, top_p=0.95, seed=3)
    q = inf.AccompanimentQueue(model, e2i, i2e, leads, primers, 4, redraw=False, **kw)
    assert q.eng.persist is not None and q.eng.persist['args'].form == (0 if kind == 'performer' else 1)
    # a second engine on the chain of launches, fed what the slots are fed (tokens, segments, positions, restarts)
    ref = inf.AccompanimentQueue(model, e2i, i2e, leads, primers, 4, redraw=False, persistent=False, **kw)
    assert ref.eng.persist is None
    ref._gargs, ref.tok, ref.segv, ref.row_reset = None, q.tok, q.segv, q.row_reset        # (its own grammar block is never launched)
    ref.eng.pos_dev = q.eng.pos_dev
    hosts = [HostJob(inf, e2i, i2e, ld, p, None, 60, False) for ld, p in zip(leads, primers)]
    graph = None
    worst, rng, polls, launches, checked = 0.0, 0.0, 0, 0, 0
    with torch.no_grad():
        while q._live() > 0:
            q.eng.check_persistent()                                      # after each poll
            polls += 1
            held = q.slot_job.cpu().tolist()
            lg = q.logits.clone()
            # the host grammar on the slot's own logits with the job's uniforms: what this launch must do to every job that draws
            want = [b for b, j in enumerate(held) if j >= 0 and len(hosts[j].s.generated) < 64 and hosts[j].consumed >= len(hosts[j].s.generated)]
            for b, j in enumerate(held):
                if j >= 0 and b not in want:
                    if len(hosts[j].s.generated) >= 64:
                        hosts[j].status = inf.ACC_WINDOW
                    else:
                        hosts[j].feed()
            drew = list(want)
            while want:
                u = torch.zeros(4, device=DEV)
                for b in want:
                    u[b] = q.U[min(hosts[held[b]].draws, q.U.shape[0] - 1), held[b]]
                words = ops.sample_nucleus(lg, 1.2, 0.95, u).cpu().tolist()
                want = [b for b in want if hosts[held[b]].offer(words[b], q.U.shape[0])]
            for b in drew:
                if hosts[held[b]].status == inf.ACC_RUNNING:
                    hosts[held[b]].feed()
            if graph is None and launches >= 1:                           # one-step graph replays from the second launch on
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side), torch.cuda.graph(graph, stream=side):
                    q.one_step()
            if graph is None:
                q.one_step()
            else:
                graph.replay()
            torch.cuda.synchronize()
            launches += 1
            st, seq = q.state.cpu().numpy(), q.seq.cpu().numpy()
            for b, j in enumerate(held):
                if j >= 0:
                    for k, v in hosts[j].state().items():
                        assert st[j, k] == v, (launches, b, j, k, st[j].tolist(), hosts[j].state())
                    assert seq[j, :len(hosts[j].s.generated)].tolist() == hosts[j].s.generated
                    checked += 1
            ref.model_step()                                              # the same tokens, segments, positions and row flags
            now = q.slot_job.cpu().tolist()
            for b, j in enumerate(now):
                if j >= 0:
                    worst = max(worst, float((q.logits[b] - ref.logits[b]).abs().max()))
                    rng = max(rng, float(ref.logits[b].max() - ref.logits[b].min()))
            assert launches < 1500
        q.eng.check_persistent()
    print('[measured] %s one-launch bf16, 9 jobs / 4 slots, %d launches (%d replayed), %d polls: slot rows against a second engine fed the same: '
          '%.4f of the logit range' % (kind, launches, launches - 2, polls, worst / rng))
    assert checked >= 100 and all(h.status != inf.ACC_RUNNING for h in hosts)
    assert worst <= 0.02 * rng


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_generate_accompaniments_with_slots_end_to_end(kind, monkeypatch):
    from emo_disentanger_amd import inference as inf, scoring
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 64)
    model = _tiny(kind, 'fp32', tls_bias=3.0)
    leads, primers = _jobs(g, 7)
    kw = dict(max_events=60, temp=1.2, top_p=0.95, seed=9)
    res, _, picks, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, slots=3, best_of=2, best_by='draws', return_scores=True, **kw)
    assert len(res) == len(picks) == len(sc) == 7
    # the 14 jobs themselves, through the loop: the candidates are those, and the picks are picks_of on their recorded means
    q = inf.AccompanimentQueue(model, e2i, i2e, [l for l in leads for _ in range(2)], [p for p in primers for _ in range(2)], 3, redraw=False,
                               scores=True, **kw)
    q.run()
    jobs = q.results(e2i, i2e, 60, False, 9)
    jsc = q.scores(jobs)
    status = q.state[:, inf.ACC_S_STATUS].cpu().tolist()
    ok = lambda r: isinstance(r, list)      # noqa: E731
    assert sum(ok(r) for r in jobs) >= 12
    for j, (r, s) in enumerate(zip(jobs, jsc)):                           # well-formed per _Stream.result(), scores aligned with ids
        if status[j] in (inf.ACC_DONE, inf.ACC_STUCK):
            ids = q.seq[j, :int(q.state[j, inf.ACC_S_LEN])].cpu().tolist()
            assert r == (ids if status[j] == inf.ACC_STUCK else ids[:-1])
        if ok(r):
            lead, primer = leads[j // 2], primers[j // 2]
            assert r[:len(primer)] == primer and e2i['PAD_None'] not in r
            assert len(s['logp']) == len(s['rank']) == len(s['entropy']) == len(r)
            given = np.isnan(s['logp'])
            assert given[:len(primer) + 2 + len(lead[0])].all() and (s['rank'][given] == -1).all() and (s['rank'][~given] >= 0).all()
            if status[j] in (inf.ACC_DONE, inf.ACC_STUCK):                  # (a job the host finished past the window records nothing there)
                assert int((~given).sum()) == int(q.state[j, inf.ACC_S_ACCEPTED]) - (status[j] == inf.ACC_DONE)      # the last draw is cut off
    want = scoring.picks_of(jobs, scoring.draw_scores_mean(jsc), 2, jsc)
    for p, w, r in zip(picks, want, res):
        assert p['chosen'] == w['chosen'] and [c if ok(c) else None for c in p['candidates']] == [c if ok(c) else None for c in w['candidates']]
        assert all((a != a and b != b) or a == b for a, b in zip(p['nll_mean'], w['nll_mean']))
        assert r == p['candidates'][p['chosen']] or not ok(r)
    # slots=None on the same arguments is the lock-step loop, as before
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **kw)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
    loop.run()
    assert plain == loop.results(e2i, i2e, 60, False, 9)
    # reported, not asserted: a job's ids at 3, 7 and 16 slots (a GEMM row may depend on the batch's row count)
    runs = [inf.generate_accompaniments(model, e2i, i2e, leads, primers, slots=s, **kw)[0] for s in (3, 7, 16)]
    same = sum(a == b == c for a, b, c in zip(*runs))
    print('[measured] %s fp32: jobs with the same ids at 3, 7 and 16 slots: %d of 7' % (kind, same))
    assert all(ok(r) or isinstance(r, Exception) for run in runs for r in run)
