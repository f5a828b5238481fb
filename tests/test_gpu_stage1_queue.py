"""GPU: stage-1 generation from a queue (emo_grammar_step, kind TXL_QUEUE; stage1_inference.LeadSheetQueue).  First what the loop is built on:
a decode step at an empty memory equals a one-token prefill, and a row whose length is reset to 0 restarts without touching its neighbours.
Then the kernel against the host grammar (HostStream of tests/test_gpu_stage1_batch.py), launch by launch, with the admissions checked after
every launch; its scores; and the whole loop under graph replay, through generate_lead_sheets(slots=) and the command line.
Bounds: fp32 logits of two routes to the same value within LOGIT_TOL x the logits' scale (tests/test_gpu_stage1_scoring.py, tests/test_gpu_generate.py);
the one-launch step against the chain within 2 % of the logit range (tests/test_gpu_stage1_one_launch.py); ids drawn with ops.sample_nucleus are exact."""
import functools
import json
import os
import pickle

import numpy as np
import pytest
import torch

from test_gpu_stage1_batch import HostStream
from test_gpu_stage1_one_launch import V, _model, _sd, _toy_vocab

pytestmark = pytest.mark.gpu
LOGIT_TOL = 2e-4
DEV = 'cuda'


def _biased_sd(seed=5, bias=3.0):
    e2i, _ = _toy_vocab()
    sd = _sd(2, seed=seed)
    for e, i in e2i.items():                                         # keys, bars and beats likely: the key rule passes and the grammar has work
        if e.startswith('Key_') or e == 'Bar_None' or e.startswith('Beat_'):
            sd['dec_out_proj.bias'][i] += bias
    return sd


@functools.lru_cache(None)
def _fp32_model(max_gen_len=320):
    return _model(2, 8, 'fp32', _biased_sd(), max_gen_len=max_gen_len)


# ------------------------------------------------------------------------------------------------ what the loop is built on
def _one_token_prefill(m, tok):
    from emo_disentanger_amd.model.plain_transformer import TXLMemory
    n = tok.numel()
    mem = TXLMemory(m, n, m._max_gen_len)
    h, _, _ = m._prefill(tok.view(1, n), mem)
    return m._logits(h.view(n, 1, -1)[:, -1].contiguous()).float().clone(), mem


def test_chain_decode_step_at_an_empty_memory_equals_a_one_token_prefill():
    from emo_disentanger_amd.model.plain_transformer import TXLMemory
    m = _fp32_model()
    tok = torch.tensor([0, 3, 57, 199, 120], device=DEV)
    with torch.no_grad():
        ref, pmem = _one_token_prefill(m, tok)
        mem = TXLMemory(m, 5, m._max_gen_len)
        got = m.decode_step(tok, mem).float().clone()
    scale = float(ref.abs().max())
    e = float((got - ref).abs().max())
    print('[measured] chain fp32, decode step at zero cached rows vs one-token prefill: %.3e (scale %.3e)' % (e, scale))
    assert mem.lens.tolist() == [1] * 5
    assert e <= LOGIT_TOL * scale
    for a, b in zip(mem.kc + mem.vc, pmem.kc + pmem.vc):           # the row the step appended is the prefill's
        assert float((a[:, 0] - b[:, 0]).abs().max()) <= LOGIT_TOL * max(1.0, float(b[:, 0].abs().max()))


def test_one_launch_step_at_an_empty_memory_equals_a_one_token_prefill():
    from emo_disentanger_amd import stage1_inference as s1
    m = _model(2, 8, 'bf16', _biased_sd(), max_gen_len=96)
    tok = torch.tensor([0, 3, 57, 199, 120], device=DEV)           # 5 rows: a padded second group
    with torch.no_grad():
        ref, _ = _one_token_prefill(m, tok)
        st = s1.OneLaunchStep(m, 5)
        got = st.step(tok).float().clone()
        st.check_persistent()
    rng = float(ref.max() - ref.min())
    e = float((got - ref).abs().max())
    print('[measured] one-launch step at zero cached rows vs one-token prefill (bf16): %.4f of the logit range' % (e / rng))
    assert st.mem.lens.tolist() == [1] * 5
    assert e <= 0.02 * rng


def test_a_row_whose_length_is_reset_restarts_and_the_others_go_on():
    # three rows; after 5 steps row 1 is reset (length 0), then 14 more steps: rows 0 and 2 cross the window of 8 at lengths 5 .. 19 while row 1
    # runs 0 .. 14.  Every row's logits are those of a memory of its own fed the same tokens: rows 0 and 2 all 19, row 1 the last 14.
    from emo_disentanger_amd.model.plain_transformer import TXLMemory
    m = _fp32_model()
    g = torch.Generator().manual_seed(9)
    toks = torch.randint(0, V - 1, (19, 3), generator=g).to(DEV)
    with torch.no_grad():
        mem = TXLMemory(m, 3, m._max_gen_len)
        got = []
        for t in range(19):
            if t == 5:
                mem.lens[1] = 0
            got.append(m.decode_step(toks[t], mem).float().clone())
        assert mem.lens.tolist() == [19, 14, 19]
        alone = {}
        for r, t0 in ((0, 0), (1, 5), (2, 0)):
            am = TXLMemory(m, 1, m._max_gen_len)
            alone[r] = [None] * t0 + [m.decode_step(toks[t, r:r + 1], am).float().clone()[0] for t in range(t0, 19)]
    scale = max(float(x.abs().max()) for x in got)
    worst = 0.0
    for t in range(19):
        for r in range(3):
            if alone[r][t] is not None:
                worst = max(worst, float((got[t][r] - alone[r][t]).abs().max()))
    print('[measured] rows at different lengths vs each row alone: %.3e (scale %.3e)' % (worst, scale))
    assert worst <= LOGIT_TOL * scale


# ------------------------------------------------------------------------------------------------ the kernel, launch by launch
NOTES = ['Note_Degree_%d' % i for i in range(1, 14)]
JOBS = [  # primer, representation, key_determine, max_bars, max_events, prompt_bars, scripted first draws (then the model's logits), the ending
    (['Emotion_Q1'], 'functional', None, 8, 12, None, ['Key_C'] + NOTES[:11], 'DONE'),                                   # max_events (fully scripted)
    (['Emotion_Q2'], 'functional', 'rule', 4, 30, None, ['Chord_0_1'], 'KEY_ERROR'),                                      # a non-Key first draw
    (['Emotion_Positive', 'Key_C', 'Bar_None'], 'functional', None, 6, 20, 1, ['PAD_None', 'Beat_2', 'Beat_1'], 'DONE'),  # the primer fed again
    (None, 'remi', None, 8, 40, None, ['Bar_None', 'Beat_7'] + ['Beat_0'] * 256, 'STUCK'),
    (['Emotion_Q4'], 'functional', 'rule', 3, 40, None, ['Key_a', 'Key_G'], 'DONE'),                                      # a key of the wrong mode
    (['Emotion_Negative', 'Key_a'], 'functional', None, 2, 36, None, ['Bar_None', 'Beat_0', 'Bar_None'], 'DONE'),         # max_bars
    (['Emotion_Q3'], 'functional', None, 8, 24, None, ['Key_e', 'Bar_None', 'EOS_None'], 'DONE'),                         # EOS
    (['Emotion_Q2'], 'functional', None, 3, 16, None, [], 'DONE'),                                                       # the model's draws only
]


class QueueRig:
    """The queue kernel and its host restatement side by side: `slots` rows of a real fp32 model (chain step) and of the host's own book of
    which slot holds which job.  launch(): script or keep the logits, predict every slot with HostStream, launch, compare, admit as the device
    did (which freed slot got which job is the device's choice; THAT the next consecutive jobs were admitted is checked), model step."""

    def __init__(self, jobs, slots, max_gen_len, scores=False, seed=13):
        from emo_disentanger_amd import ops, stage1_inference as s1
        from emo_disentanger_amd.model.plain_transformer import TXLMemory
        self.ops, self.s1 = ops, s1
        self.m = _fp32_model(max_gen_len)
        self.e2i, self.i2e = _toy_vocab()
        self.jobs, self.slots, n = jobs, slots, len(jobs)
        self.hosts = [HostStream(self.e2i, self.i2e, p, rep, kd, mb, me, pb, 1) for p, rep, kd, mb, me, pb, _, _ in jobs]
        self.scripts = [[self.e2i[w] for w in j[6]] for j in jobs]
        flags, beat = s1.event_tables(self.i2e, V)
        W = 300
        seq, params, state = np.zeros((n, W), np.int64), np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
        for i, (h, j) in enumerate(zip(self.hosts, jobs)):
            seq[i, :h.plen] = h.sheet.tokens
            params[i, :6] = j[3], j[4], h.plen, h.keyed, h.rule, s1.emotion_mode(self.i2e, h.sheet.tokens[0])
            state[i, [s1.S_STATUS, s1.S_LEN, s1.S_BARS, s1.S_FEED]] = h.status, h.plen, h.sheet.bars, 1
        T = lambda a: torch.from_numpy(a).to(DEV)       # noqa: E731
        self.seq, self.params, self.state, self.ev_flags, self.ev_beat = T(seq), T(params), T(state), T(flags), T(beat)
        self.running = torch.tensor([self.live()], dtype=torch.int32, device=DEV)
        self.mem = TXLMemory(self.m, slots, max_gen_len)
        self.U = torch.rand(max_gen_len, n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
        self.tok = T(seq[:1, 0].repeat(slots))
        self.logits = torch.zeros(slots, V, device=DEV)
        self.slot_job = torch.full((slots,), -1, dtype=torch.int32, device=DEV)
        self.queue_head = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.job_steps = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        self.tabs = ops.draw_score_tables(self.seq) if scores else {}
        self.tabs0 = {k: t.clone() for k, t in self.tabs.items()}
        self.book = [-1] * slots                     # the host's slot_job
        self.head, self.admitted, self.steps, self.launches, self.drained = 0, [], {}, 0, None
        self.open = [j for j, h in enumerate(self.hosts) if h.status == s1.RUNNING]      # a job closed before the run is passed over
        self.drawn_cells = {}                        # (job, column) -> (logits row, token) of every accepted draw

    def live(self):
        return sum(h.status == self.s1.RUNNING for h in self.hosts)

    def launch(self):
        ops, s1, slots = self.ops, self.s1, self.slots
        lens = self.mem.lens.cpu().tolist()
        full = [lens[b] >= self.mem.max_len for b in range(slots)]
        draws = [b for b in range(slots) if self.book[b] >= 0 and not full[b] and self.hosts[self.book[b]].wants_draw()]
        for b in draws:                               # a scripted draw: a one-hot row, which the nucleus keeps whatever u is
            h, sc = self.hosts[self.book[b]], self.scripts[self.book[b]]
            if h.draws < len(sc):
                self.logits[b].zero_()
                self.logits[b, sc[h.draws]] = 60.0
        u = torch.zeros(slots, device=DEV)
        for b in draws:
            u[b] = self.U[self.hosts[self.book[b]].draws, self.book[b]]       # draw d of JOB j: row d, column j
        w_main = ops.sample_nucleus(self.logits, 1.2, 0.9, u).cpu().tolist()
        w_key = ops.sample_nucleus(self.logits, s1.KEY_TEMP, s1.KEY_TOP_P, u).cpu().tolist()
        lg = self.logits.cpu().numpy().copy()
        ops.txl_queue_step(self.logits, 1.2, 0.9, s1.KEY_TEMP, s1.KEY_TOP_P, self.U, self.ev_flags, self.ev_beat, self.params, self.state, self.seq,
                           self.tok, self.running, self.slot_job, self.queue_head, self.mem.lens, self.mem.max_len, job_steps=self.job_steps,
                           **self.tabs)
        self.launches += 1
        where = self.launches
        st, sq, tk = self.state.cpu().numpy(), self.seq.cpu().numpy(), self.tok.cpu().numpy()
        sj, ln = self.slot_job.cpu().tolist(), self.mem.lens.cpu().tolist()
        freed = []
        for b in range(slots):
            j = self.book[b]
            if j < 0:
                freed.append(b)
                continue
            h = self.hosts[j]
            if full[b]:
                h.status = s1.MEM_FULL
            else:
                before = len(h.sheet.tokens)
                h.step((w_key if h.key_step() else w_main)[b] if b in draws else None)
                if len(h.sheet.tokens) > before:
                    self.drawn_cells[(j, before)] = (lg[b], h.sheet.tokens[before])
            for k, v in h.state().items():            # every state word of the job, ids included
                assert st[j, k] == v, (where, b, j, k, st[j].tolist(), h.state())
            assert sq[j, :len(h.sheet.tokens)].tolist() == h.sheet.tokens, (where, b, j)
            if h.status == s1.RUNNING:
                assert sj[b] == j and tk[b] == h.tok and st[j, s1.S_FEED] == h.feed and ln[b] == lens[b], (where, b, j)
            else:
                self.steps[j] = lens[b]
                freed.append(b)
        # admissions: the freed slots hold the next consecutive open jobs from the head (in any order), each at length 0 with its first token out
        want = self.open[self.head:self.head + len(freed)]
        got = sorted(sj[b] for b in freed if sj[b] >= 0)
        assert got == want, (where, freed, sj, self.head)
        for b in freed:
            assert ln[b] == 0, (where, b, ln)            # admitted or free: the row starts again
            self.book[b] = sj[b]
            if sj[b] >= 0:
                assert tk[b] == self.hosts[sj[b]].sheet.tokens[0] and st[sj[b], s1.S_FEED] == 1, (where, b)
                self.hosts[sj[b]].tok = int(tk[b])
        self.head += len(want)
        self.admitted += want
        assert int(self.queue_head.item()) <= len(self.hosts) + slots
        assert int(self.running.item()) == self.live(), where
        with torch.no_grad():
            self.m.decode_step(self.tok, self.mem, logits_out=self.logits)

    def run(self, limit):
        self.launch()                                     # the first launch admits, nothing else
        assert self.admitted == self.open[:self.slots]
        while self.live() > 0:
            self.launch()
            assert self.launches < limit
        self.drained = self.launches                      # (launches behind the drain change nothing this count is compared with)
        return self


@functools.lru_cache(None)
def _stepped():
    return QueueRig(JOBS, 3, 320, scores=True).run(700)


def test_queue_kernel_matches_the_host_grammar_and_admits_in_order():
    s1 = _stepped().s1
    rig = _stepped()
    names = {'DONE': s1.DONE, 'STUCK': s1.STUCK, 'KEY_ERROR': s1.KEY_ERROR}
    assert [h.status for h in rig.hosts] == [names[j[7]] for j in JOBS]
    assert rig.admitted == list(range(len(JOBS)))                        # every job exactly once
    for i, (h, sc) in enumerate(zip(rig.hosts, rig.scripts)):
        assert h.draws >= len(sc), i                                     # every scripted word was drawn
    # the endings that were scripted
    assert len(rig.hosts[0].sheet.tokens) == 13 and rig.hosts[5].sheet.bars == 2 and rig.hosts[6].sheet.tokens[-1] == rig.e2i['EOS_None']
    assert rig.hosts[2].draws > rig.hosts[2].sheet.accepted >= 1          # the 3-token primer was fed again after its PAD
    assert max(rig.steps.values()) > 8 + 1                                # rows went past the window of 8
    # after the drain: every slot free, length 0, and it stays so
    assert rig.book == [-1] * 3
    head = int(rig.queue_head.item())
    for _ in range(3):
        rig.launch()
        assert rig.mem.lens.tolist() == [1] * 3                          # (0 after the launch — checked inside —, 1 after the model step)
    assert int(rig.queue_head.item()) == head and rig.slot_job.tolist() == [-1] * 3
    # the launches a job held its slot, as the kernel wrote them, and the plan they give
    assert rig.job_steps.tolist() == [rig.steps[j] for j in range(len(JOBS))]
    assert s1.queue_plan(rig.job_steps.tolist(), 3)[0] == rig.drained


def _check_score_cells(ops, tabs_d, tabs0, drawn_cells):
    """drawn_cells: (table row, column) -> (the logits row the draw was made from, the accepted id).  Those cells hold emo_token_scores of the
    row (ranks equal; logp, entropy within 2 x row_tol, the bound tests/test_gpu_draw_scores.py holds the pair to); no other cell changed."""
    from test_gpu_draw_scores import row_tol
    cells = sorted(drawn_cells)
    rows = torch.from_numpy(np.stack([drawn_cells[c][0] for c in cells])).to(DEV)
    toks = torch.tensor([drawn_cells[c][1] for c in cells], device=DEV)
    ts = ops.token_scores(rows, toks, -100, want=('rank', 'entropy'))
    nll, rank, ent = ts['nll'].cpu().numpy(), ts['rank'].cpu().numpy(), ts['entropy'].cpu().numpy()
    tabs = {k: t.cpu().numpy() for k, t in tabs_d.items()}
    written = np.zeros(tabs['tok_rank'].shape, bool)
    for i, (j, c) in enumerate(cells):
        written[j, c] = True
        tol = 2 * row_tol(drawn_cells[(j, c)][0])
        assert tabs['tok_rank'][j, c] == rank[i], (j, c)
        assert abs(float(tabs['tok_logp'][j, c]) + float(nll[i])) <= tol and abs(float(tabs['tok_entropy'][j, c]) - float(ent[i])) <= tol, (j, c)
    for k, t in tabs_d.items():                                          # every other cell holds what the caller put there
        same = (t.view(torch.int32) == tabs0[k].view(torch.int32)).cpu().numpy()
        assert np.array_equal(~same, written), k


def test_queue_kernel_scores_exactly_the_drawn_cells_of_the_jobs_tables():
    rig = _stepped()
    assert len(rig.drawn_cells) >= 22                                    # (what the scripts alone guarantee)
    _check_score_cells(rig.ops, rig.tabs, rig.tabs0, rig.drawn_cells)


def test_a_job_that_fills_its_row_ends_with_mem_full_and_the_slot_goes_on():
    # max_gen_len 16: job 0 draws notes until its row is full (16 tokens fed), the two jobs behind it end on their own
    s1 = _stepped().s1
    notes = ['Key_C'] + [NOTES[i % 13] for i in range(40)]
    jobs = [(['Emotion_Q1'], 'functional', None, 8, 60, None, notes, 'MEM_FULL'),
            (['Emotion_Q2'], 'functional', None, 8, 60, None, ['Key_a', 'EOS_None'], 'DONE'),
            (['Emotion_Q3'], 'functional', None, 8, 5, None, ['Key_e'] + NOTES[:4], 'DONE')]
    rig = QueueRig(jobs, 2, 16).run(60)
    assert [h.status for h in rig.hosts] == [s1.MEM_FULL, s1.DONE, s1.DONE]
    assert rig.job_steps.tolist() == [16, 2, 5] and rig.hosts[0].draws == 15 and len(rig.hosts[0].sheet.tokens) == 16
    assert rig.admitted == [0, 1, 2] and rig.drained == s1.queue_plan([16, 2, 5], 2)[0] == 17
    assert int(rig.mem.lens.max()) <= 16


def test_jobs_closed_before_the_run_are_passed_over_in_the_queue():
    # jobs 1 and 2 are closed on the host (the primer already holds max_bars bars): status DONE before the first launch, never RUNNING, so they
    # are not in the running count.  A slot that comes to them in the queue goes on to the next open job in the same launch.
    s1 = _stepped().s1
    closed = (['Emotion_Positive', 'Key_C', 'Bar_None'], 'functional', None, 1, 30, 1, [], 'DONE')
    jobs = [(['Emotion_Q1'], 'functional', None, 8, 3, None, ['Key_C'] + NOTES[:2], 'DONE'), closed, closed,
            (['Emotion_Q2'], 'functional', None, 8, 60, None, ['Key_a', 'EOS_None'], 'DONE'),
            (['Emotion_Q3'], 'functional', None, 8, 4, None, ['Key_e'] + NOTES[:3], 'DONE'), closed]
    rig = QueueRig(jobs, 2, 32)
    assert rig.open == [0, 3, 4] and int(rig.running.item()) == 3
    rig.run(40)
    assert rig.admitted == [0, 3, 4] and all(h.status == s1.DONE for h in rig.hosts)
    assert rig.job_steps.tolist() == [3, -7, -7, 2, 4, -7]               # a closed job held no slot: its cell keeps the caller's value
    assert rig.drained == s1.queue_plan([3, 2, 4], 2)[0] == 7
    st = rig.state.cpu().numpy()
    assert st[[1, 2, 5], s1.S_DRAWS].tolist() == [0, 0, 0] and st[[1, 2, 5], s1.S_LEN].tolist() == [3, 3, 3]
    assert int(rig.queue_head.item()) == 6 and rig.slot_job.tolist() == [-1, -1]


def test_txl_kind_is_unchanged_with_the_queue_fields_null():
    # The TXL kind on a block whose queue fields are NULL / 0, against the host grammar on the same draws (the parent's behaviour, restated):
    # six launches on three streams, one of them feeding a 3-token primer, every id and state word.
    from emo_disentanger_amd import ops, stage1_inference as s1
    e2i, i2e = _toy_vocab()
    streams = [(['Emotion_Q1'], 'functional', None, 4, 30, None), (['Emotion_Positive', 'Key_C', 'Bar_None'], 'functional', None, 4, 30, 1),
               (['Emotion_Q2'], 'functional', 'rule', 4, 30, None)]
    hosts = [HostStream(e2i, i2e, *s, 1) for s in streams]
    flags, beat = s1.event_tables(i2e, V)
    seq, params, state = np.zeros((3, 40), np.int64), np.zeros((3, 8), np.int32), np.zeros((3, 8), np.int32)
    for i, (h, s) in enumerate(zip(hosts, streams)):
        seq[i, :h.plen] = h.sheet.tokens
        params[i, :6] = s[3], s[4], h.plen, h.keyed, h.rule, s1.emotion_mode(i2e, h.sheet.tokens[0])
        state[i, [s1.S_STATUS, s1.S_LEN, s1.S_BARS, s1.S_FEED]] = h.status, h.plen, h.sheet.bars, 1
    T = lambda a: torch.from_numpy(a).to(DEV)       # noqa: E731
    seq_d, params_d, state_d = T(seq), T(params), T(state)
    U = torch.rand(16, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    tok, running = torch.full((3,), -1, dtype=torch.long, device=DEV), torch.tensor([3], dtype=torch.int32, device=DEV)
    tabs = ops.draw_score_tables(seq_d)                                  # the scores path of the shared step, through kind TXL
    tabs0, cells = {k: t.clone() for k, t in tabs.items()}, {}
    args, held = ops.GrammarStep(kind=ops.GRAMMAR_TXL), {}
    lg = torch.empty(3, V, device=DEV)
    ops.block_set(args, held, n_rows=3, n_token=V, ld_u=3, temperature=1.2, top_p=0.9, key_temperature=1.1, key_top_p=0.97, logits=lg, u_steps=U,
                  ev_flags=T(flags), ev_beat=T(beat), params=params_d, state=state_d, seq=seq_d, tok_out=tok, running=running, **tabs)
    assert args.slot_job is None and args.queue_head is None and args.mem_lens is None and args.job_steps is None and args.n_jobs == 0
    logits = torch.randn(6, 3, V, device=DEV, generator=torch.Generator(device=DEV).manual_seed(4)) * 2.0
    logits[:, :, [e2i['EOS_None'], e2i['PAD_None']]] = -60.0
    logits[:, :, [i for e, i in e2i.items() if e.startswith('Key_')]] += 4.0
    for t in range(6):
        lg.copy_(logits[t])
        u = torch.stack([U[min(h.draws, 15), i] for i, h in enumerate(hosts)])
        w_main = ops.sample_nucleus(lg, 1.2, 0.9, u).cpu().tolist()
        w_key = ops.sample_nucleus(lg, 1.1, 0.97, u).cpu().tolist()
        ops.grammar_step(args)
        for i, h in enumerate(hosts):
            before = len(h.sheet.tokens)
            h.step((w_key if h.key_step() else w_main)[i] if h.wants_draw() else None)
            if len(h.sheet.tokens) > before:
                cells[(i, before)] = (logits[t, i].cpu().numpy(), h.sheet.tokens[before])
        st, sq, tk = state_d.cpu().numpy(), seq_d.cpu().numpy(), tok.cpu().numpy()
        for i, h in enumerate(hosts):
            for k, v in h.state().items():
                assert st[i, k] == v, (t, i, k)
            assert sq[i, :len(h.sheet.tokens)].tolist() == h.sheet.tokens
            if h.status == s1.RUNNING:
                assert tk[i] == h.tok and st[i, s1.S_FEED] == h.feed
    assert sum(h.draws for h in hosts) >= 8
    _check_score_cells(ops, tabs, tabs0, cells)
    assert len(cells) >= 4


# ------------------------------------------------------------------------------------------------ the whole loop
PRIMERS10 = [  # primer, representation, key_determine, max_bars, max_events, prompt_bars
    (['Emotion_%s' % e], 'functional', kd, mb, me, None) for e, kd, mb, me in
    [('Q1', None, 3, 40), ('Q2', 'rule', 4, 36), ('Positive', None, 2, 24), ('Negative', 'rule', 3, 44), ('Q3', None, 3, 12), ('Q4', 'rule', 2, 30),
     ('Q1', None, 4, 48), ('Q2', None, 3, 16)]
] + [(['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_0_1'], 'functional', None, 3, 44, 1), (None, 'remi', None, 2, 30, None)]


def _kw10(**more):
    cols = list(zip(*PRIMERS10))
    kw = dict(representation=list(cols[1]), key_determine=list(cols[2]), max_bars=list(cols[3]), max_events=list(cols[4]),
              prompt_bars=list(cols[5]), temp=1.2, top_p=0.9, seed=7)
    kw.update(more)
    return list(cols[0]), kw


def _check_grammar(s1, i2e, results, kws):
    for r, (_, _, _, mb, me, pb) in zip(results, PRIMERS10):
        assert r is None or isinstance(r, (list, ValueError)), r
        if not isinstance(r, list):
            continue
        assert len(r) <= me
        beat, bars = 0, pb or 0
        for w in r[1:]:
            e = i2e[w]
            assert e != 'PAD_None'
            if 'Beat' in e:
                assert s1.beat_position(e) >= beat
                beat = s1.beat_position(e)
            if 'Bar' in e:
                bars, beat = bars + 1, 0
        assert bars <= mb


@pytest.mark.parametrize('step', ['chain', 'one_launch'])
def test_whole_loop_under_graph_replay(step):
    from emo_disentanger_amd import stage1_inference as s1
    e2i, i2e = _toy_vocab()
    m = _fp32_model(96) if step == 'chain' else _model(2, 8, 'bf16', _biased_sd(), max_gen_len=96)
    primers, kw = _kw10(step=step)
    got, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, slots=3, **kw)
    again, _, sc = s1.generate_lead_sheets(m, e2i, i2e, primers, slots=3, return_scores=True, **kw)
    plain = lambda rs: [r if isinstance(r, list) else type(r).__name__ for r in rs]      # noqa: E731
    assert plain(got) == plain(again)
    _check_grammar(s1, i2e, got, kw)
    assert sum(isinstance(r, list) for r in got) >= 5
    for r, s, p in zip(again, sc, primers):
        assert (s is None) == (not isinstance(r, list))
        if s is not None:                                                # every id behind the primer was drawn, and has its figures
            plen = 1 if p is None else len(p)
            assert len(s['logp']) == len(r) and np.isnan(s['logp'][:plen]).all() and np.isfinite(s['logp'][plen:]).all()
    # the loop itself: one-step graphs, so the host's count of launches is exact; then the default 16-step graphs
    q1 = s1.LeadSheetQueue(m, e2i, i2e, primers, 3, **kw)
    q1.run(use_graph=True, steps_per_graph=1)
    assert q1.replayed[0] > 0                                            # (replays did run)
    st = q1.state.cpu().numpy()
    assert int(q1.running.item()) == 0 and (st[:, s1.S_STATUS] != s1.RUNNING).all()
    assert plain(q1.results()) == plain(got)
    steps = q1.job_steps()
    # a job whose primer has one token held its slot one launch per draw
    assert [steps[j] for j in range(8)] == st[:8, s1.S_DRAWS].tolist()
    launches, occ = s1.queue_plan(steps, 3)
    print('[measured] %s: 10 jobs through 3 slots in %d launches, occupancy %.3f; lock-step 10 rows: %d steps' % (step, launches, occ, max(steps)))
    assert q1.launches == launches
    assert q1.slot_job.tolist() == [-1] * 3 and int(q1.queue_head.item()) <= 10 + 3
    q16 = s1.LeadSheetQueue(m, e2i, i2e, primers, 3, **kw)
    q16.run(use_graph=True)
    assert plain(q16.results()) == plain(got) and q16.job_steps() == steps
    assert launches <= q16.launches < launches + 16                      # a 16-step replay ends at most 15 launches past the drain
    assert int(q16.mem.lens.max()) <= 96


def test_a_jobs_result_does_not_depend_on_the_slots():
    # fp32 chain: 3 slots against a slot per job and against more slots than jobs.  Every job's result is the same list of ids, whatever
    # slot it ran in and whatever ran beside it.  (What a slot's logits ARE is the test below: each job against a memory of its own.)
    from emo_disentanger_amd import stage1_inference as s1
    e2i, i2e = _toy_vocab()
    m = _fp32_model(96)
    primers, kw = _kw10()
    a, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, slots=3, **kw)
    b, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, slots=10, **kw)
    c, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, slots=16, **kw)
    plain = lambda rs: [r if isinstance(r, list) else type(r).__name__ for r in rs]      # noqa: E731
    same = [x == y == z for x, y, z in zip(plain(a), plain(b), plain(c))]
    print('[measured] jobs with the same result at 3, 10 and 16 slots: %d of 10' % sum(same))
    assert all(same), same


def test_one_launch_refusals_count_the_slots():
    from emo_disentanger_amd import stage1_inference as s1
    from emo_disentanger_amd._lib import EmoError
    e2i, i2e = _toy_vocab()
    m = _model(1, 8, 'bf16', max_gen_len=32)
    with pytest.raises(EmoError, match='1 to 32 streams'):
        s1.generate_lead_sheets(m, e2i, i2e, [['Emotion_Q1']] * 4, max_bars=2, max_events=8, representation='remi', step='one_launch', slots=33)
    res, _ = s1.generate_lead_sheets(m, e2i, i2e, [['Emotion_Q1']] * 40, max_bars=2, max_events=8, representation='remi', step='one_launch', slots=4)
    assert len(res) == 40 and all(r is None or isinstance(r, list) for r in res)      # 40 jobs are fine: the slots are what the launch holds


def test_command_line_with_slots_writes_lead_sheets_that_stage2_reads(tmp_path):
    import yaml
    from emo_disentanger_amd import inference, stage1_inference as s1
    from oracle.txl_ref import make_state_dict_txl
    g = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'txl_generate.json')))
    events = [e for e in g['events'] if e != 'PAD_None']
    vocab = tmp_path / 'dictionary.pkl'
    pickle.dump(({e: i for i, e in enumerate(events)}, {i: e for i, e in enumerate(events)}), open(vocab, 'wb'))
    sd = make_state_dict_txl(len(events) + 1, 2, 4, 64, 128, seed=3, scale=2.0)
    for e in events:                                              # keys and bars likely, so that the key rule passes and bars appear
        if e.startswith('Key_') or e == 'Bar_None':
            sd['dec_out_proj.bias'][events.index(e)] += 6.0
    torch.save(sd, tmp_path / 'params.pt')
    conf = {'device': 'cuda', 'model': {'d_word_embed': 64, 'pre_lnorm': True,
                                        'decoder': {'n_layer': 2, 'n_head': 4, 'd_model': 64, 'd_ff': 128, 'dropout': 0.1, 'mem_len': 0, 'tgt_len': 64}},
            'data': {'vocab_path': str(tmp_path / 'dictionary.pkl')}}
    yaml.safe_dump(conf, open(tmp_path / 'conf.yaml', 'w'))
    out = tmp_path / 'gen'
    s1.main(['-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '-m', 'lead_sheet', '-i', str(tmp_path / 'params.pt'), '-o', str(out),
             '-n', '3', '--slots', '2', '--dtype', 'fp32'])
    files = sorted(os.listdir(out))
    assert files and all(f.startswith('samp_0') and f.endswith('_roman.txt') and ('Positive' in f or 'Negative' in f) for f in files)
    e2i, _, _ = s1.read_vocab(str(vocab))
    for f in files:
        lines = open(out / f).read().splitlines()
        assert not any(x.startswith('Emotion_') for x in lines[:1])
        key, bars = inference.read_lead_sheet(str(out / f), e2i)
        assert key.startswith('Key_') and bars and all(b[0] == e2i['Bar_None'] for b in bars)


# ------------------------------------------------------------------------------------------------ every job against a memory of its own
RESTATED = [  # primer, max_events: one- and two-token primers, more jobs than slots, lengths past the model's window
    (['Emotion_Q1'], 100), (['Emotion_Q2'], 24), (['Emotion_Negative', 'Key_a'], 90), (['Emotion_Positive'], 12), (['Emotion_Negative'], 100),
    (['Emotion_Q1'], 40), (['Emotion_Positive', 'Key_C'], 30), (['Emotion_Q2'], 80), (['Emotion_Q1'], 18),
    (['Emotion_Positive'], 100), (['Emotion_Q2', 'Key_a'], 70), (['Emotion_Negative'], 100), (['Emotion_Q1'], 100), (['Emotion_Positive'], 60),
]


def test_a_slots_logits_are_those_of_a_memory_of_the_jobs_own():
    # The queue loop stepped by hand, 14 jobs through 3 slots, on the tiny fp32 generator of tests/test_gpu_generation_scores.py (window 16).  Beside it runs
    # the restatement, which shares nothing with the queue: ONE-ROW TXLMemory per job, created when the job is admitted and fed, by plain
    # decode_step calls, exactly the token its slot was fed in every launch — the first token, a re-fed token after a rejection and a re-fed
    # primer included.  At every draw the slot's logits row is held to the job's own row, and the recorded log-probability of every accepted
    # draw to float64 on the job's own row at the bound of that file (2 x its measured ('chain', 'steps') figure: there the two sides are rows
    # of two batches of equal height, here a row of a batch of 3 beside neighbours at other lengths against a batch of 1).  Ids: the accepted
    # id is drawn again from the job's own row with ops.sample_nucleus and the job's uniform; it is compared wherever the two rows are
    # bit-equal (no margin is needed there), which has to hold for at least half of the accepted draws.
    from emo_disentanger_amd import ops, stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import TXLMemory
    from test_gpu_generation_scores import STAGE1_MEASURED, Ranks, bound, log_softmax64, margin
    from test_gpu_stage1_scoring import _generator_fixture
    full, e2i, i2e = _generator_fixture()
    # (that generator with a window of 16 in place of 64, so that the longer jobs' rows slide past it: the same weights, vocabulary and logits' scale)
    m = type(full)(full.d_word_embed, full.vocab_size, full.dec_n_layer, full.dec_n_head, full.dec_d_model, full.dec_d_ff, 16, 16, dec_dropout=0.1,
                   pre_lnorm=True, compute_dtype='fp32')
    m.load_state_dict(full.state_dict())
    m = m.cuda().eval()
    b_steps = STAGE1_MEASURED[('chain', 'steps')]
    q = s1.LeadSheetQueue(m, e2i, i2e, [p for p, _ in RESTATED], 3, max_bars=32, max_events=[me for _, me in RESTATED], temp=1.2, top_p=0.9,
                          representation='functional', seed=11, scores=True)
    n = q.n
    own_mem, own = [None] * n, [None] * n                                 # per job: its memory, the logits of its last step
    ranks, err, err_logits, hits, exact, ids_equal, refed, launches = Ranks(), 0.0, 0.0, 0, 0, 0, 0, 0
    params = q.params.cpu().numpy()
    with torch.no_grad():
        while q._live() > 0:
            before, held = q.state.cpu().numpy().copy(), q.slot_job.cpu().tolist()
            slot_logits = q.logits.clone()
            q.grammar()
            launches += 1
            after, seq, now, fed = q.state.cpu().numpy(), q.seq.cpu().numpy(), q.slot_job.cpu().tolist(), q.tok.cpu().tolist()
            for b, j in enumerate(held):
                if j < 0 or after[j, s1.S_DRAWS] == before[j, s1.S_DRAWS]:
                    continue
                d = float((slot_logits[b] - own[j]).abs().max())          # every draw, rejected ones included
                err_logits = max(err_logits, d)
                if after[j, s1.S_ACCEPTED] == before[j, s1.S_ACCEPTED]:
                    refed += 1
                    continue
                c = int(before[j, s1.S_LEN])
                tok = int(seq[j, c])
                lsm, l64 = log_softmax64(own[j])
                e = abs(float(q.score_tables['tok_logp'][j, c].item()) - lsm[tok])
                err = max(err, e)
                ranks.add(q.score_tables['tok_rank'][j, c].item(), (l64 > l64[tok]).sum() + (l64[:tok] == l64[tok]).sum(), margin(l64, tok), 2 * b_steps)
                hits += 1
                if d == 0.0:
                    exact += 1
                    key = bool(params[j, s1.P_KEYED]) and c == 1
                    u = q.U[int(before[j, s1.S_DRAWS]), j].reshape(1)
                    w = ops.sample_nucleus(own[j].view(1, -1).contiguous(), s1.KEY_TEMP if key else 1.2, s1.KEY_TOP_P if key else 0.9, u)
                    ids_equal += int(w.item()) == tok
            if q._live() == 0:
                break
            m.decode_step(q.tok, q.mem, logits_out=q.logits)
            for b, j in enumerate(now):
                if j < 0:
                    continue
                if held[b] != j:                                          # admitted in this launch: a memory of its own, from nothing
                    assert own_mem[j] is None and fed[b] == seq[j, 0]
                    own_mem[j] = TXLMemory(m, 1, m._max_gen_len)
                own[j] = m.decode_step(torch.tensor([fed[b]], device=DEV), own_mem[j]).float().clone()[0]
            assert launches < 2000
    st = q.state.cpu().numpy()
    assert (st[:, s1.S_STATUS] != s1.RUNNING).all() and all(x is not None for x in own_mem)
    for j in range(n):                                                    # the job's own memory was fed as many tokens as the kernel counted
        assert int(own_mem[j].lens.item()) == q.job_steps()[j], j
    print('[measured] queue, 14 jobs / 3 slots, each job against a memory of its own: %d accepted draws (%d draws rejected and re-fed), '
          'max |slot logits - own logits| = %.3e over every draw, bit-equal rows at %d accepted draws, ids equal at %d of them'
          % (hits, refed, err_logits, exact, ids_equal))
    assert hits >= 100 and refed >= 5 and max(q.job_steps()) > m.dec_mem_len + 1      # (rows went past the model's window)
    assert 2 * exact >= hits and ids_equal == exact
    ranks.check('queue against each job\'s own memory')
    bound(b_steps, err, 'queue, chain fp32, each job\'s own memory in float64')


@pytest.mark.parametrize('best_by', ['draws', 'forward'])
def test_best_of_picks_per_job_through_the_queue(best_by):
    # 3 primers x 3 candidates = 9 jobs through 4 slots: candidate c of primer i is job 3 i + c, the picks are made from the jobs' results (and,
    # by 'draws', from the jobs' score tables) exactly as from the streams of a lock-step batch.
    from emo_disentanger_amd import scoring, stage1_inference as s1
    from test_gpu_stage1_scoring import _generator_fixture
    m, e2i, i2e = _generator_fixture()
    primers = [['Emotion_Q1'], ['Emotion_Negative', 'Key_a'], ['Emotion_Positive']]
    kw = dict(max_bars=4, max_events=[40, 24, 32], temp=1.2, top_p=0.9, representation='functional', seed=11)
    res, _, picks, sc = s1.generate_lead_sheets(m, e2i, i2e, primers, best_of=3, best_by=best_by, return_scores=True, slots=4, **kw)
    jobs, _, jsc = s1.generate_lead_sheets(m, e2i, i2e, [p for p in primers for _ in range(3)], max_bars=4, max_events=[40] * 3 + [24] * 3 + [32] * 3,
                                           temp=1.2, top_p=0.9, representation='functional', seed=11, return_scores=True, slots=4)
    ok = lambda r: isinstance(r, list)      # noqa: E731
    assert len(res) == len(picks) == 3 and sum(ok(r) for r in jobs) >= 6
    want = scoring.draw_scores_mean(jsc) if best_by == 'draws' else scoring.lead_sheet_candidate_scores(m, jobs, [len(p) for p in primers for _ in range(3)])
    for i, p in enumerate(picks):
        cands = jobs[3 * i:3 * i + 3]
        assert [c if ok(c) else None for c in p['candidates']] == [c if ok(c) else None for c in cands]
        nll = want[3 * i:3 * i + 3]
        assert all((a != a and b != b) or a == b for a, b in zip(p['nll_mean'], nll)), (p['nll_mean'], nll)
        assert p['chosen'] == scoring.best_of(nll) and (res[i] == cands[p['chosen']] if ok(res[i]) else not any(ok(c) for c in cands))
        if ok(res[i]):
            assert np.array_equal(sc[i]['rank'], jsc[3 * i + p['chosen']]['rank'])
    assert len({tuple(c) for c in jobs[:3] if ok(c)}) >= 2               # the candidates of a primer drew from different uniform columns
