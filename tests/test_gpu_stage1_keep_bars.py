"""GPU: kept bars in the stage-1 device draw (emo_grammar_step, kinds TXL and TXL_QUEUE: keep_tok / keep_beg / keep_end / n_keep / keep_bar /
keep_left, params words KEEP0 / KEEP_BARS), kernel level, on synthetic fp32 logits and a small synthetic grammar.  Eight rows, a boosted logit
scripts every draw (the d-th draw of a row takes the d-th word of its script), and after EVERY launch tok_out, state, seq, running and
keep_left equal the host rule (stage1_inference._LeadSheet with keep, stepped by Host below) driven by the same words, bit for bit:
  row 0  a key rejected under the key rule and one accepted, a rejected Beat, a chain of two kept bars behind a drawn one, a Beat rejected
         directly behind the forced Bar (the forced Bar is fed again), max_bars;                        row 7: its twin on an Emotion_None primer
  row 1  a three-token primer fed beyond the common prefix, a PAD with nothing accepted (the primer again), an empty kept bar, EOS;
  row 2  a kept last bar that fills the row to its last column: the forced Bar ends the piece (max_bars) inside the chain;
  row 3  max_events inside a kept bar;
  row 4  a chain one token too long for ld_seq: OVERFLOW with the row, LEN, BARS, ACCEPTED (and BEAT, FAILED, DRAWS) as before the draw;
  row 5  a keep_end beyond n_keep (written behind block_set's back): OVERFLOW likewise;
  row 6  DONE before the first launch.
The same with a ban and per-stream temp / top_p; with rows 0 / 7 as a guided pair against the unguided launch on host-combined logits; with the
score tables (only the drawn tokens' cells are written, the kept cells keep the pre-fill); as seven jobs through three slots of kind TXL_QUEUE
(ids of the lock-step run, job_steps with the kept tokens, MEM_FULL for a kept run longer than mem_rows); and with the tables NULL both kinds
leave what the host rule without keep leaves, and what the one-shot wrappers leave."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N, WIDTH, N_U, LAUNCHES = 8, 48, 64, 24
EMO_POS, EMO_NEG, EMO_NONE, KEY_MAJ, KEY_MIN, BAR, PAD, EOS, BEAT0 = 0, 1, 2, 3, 4, 5, 6, 7, 8
BEAT_NEG = 23                                     # 'Beat_-1': a Beat below every position, rejected wherever it is drawn
NOTE0 = 24
BOOST = 60.0
TABLES = ('tok_logp', 'tok_rank', 'tok_entropy')
ROW_TOL = 1e-5                                    # tests/test_gpu_draw_scores.py: absolute, per row, at |l| < 16, scaled by the row's ulp above that
ULP16 = float(np.spacing(np.float32(15.99)))


def B(k):
    return BEAT0 + k


def NOTE(k):
    return NOTE0 + k % 9                          # (ids 24 .. 32: inside the smallest vocabulary)


def vocab(V):
    names = {EMO_POS: 'Emotion_Positive', EMO_NEG: 'Emotion_Negative', EMO_NONE: 'Emotion_None', KEY_MAJ: 'Key_C', KEY_MIN: 'Key_c', BAR: 'Bar_None',
             PAD: 'PAD_None', EOS: 'EOS_None', BEAT_NEG: 'Beat_-1'}
    for k in range(15):
        names[B(k)] = 'Beat_%d' % k
    for i in range(NOTE0, V):
        names[i] = 'Note_%d' % i
    return {e: i for i, e in names.items()}, names


LONG = [NOTE(k) for k in range(45)]
# primer, keyed, key rule, emotion mode, max_bars, max_events, keep, bars whose range is broken on the device, the script of its draws
ROWS = [
    ([EMO_POS], 1, 1, 1, 5, 1000, [None, [B(2), NOTE(1)], [NOTE(2)]], (),
     [KEY_MIN, KEY_MAJ, NOTE(0), BAR, B(3), NOTE(1), B(1), BAR, BEAT_NEG, B(1), NOTE(3), BAR]),
    ([EMO_NEG, KEY_MIN, NOTE(0)], 1, 0, 2, 3, 1000, [[], None], (), [PAD, BAR, B(4), B(2), NOTE(5), EOS]),
    ([EMO_NEG], 0, 0, 2, 3, 1000, [None, LONG[:43]], (), [BAR, NOTE(1), BAR]),        # (max_bars 3: bars 0 and 1, the third Bar closes the piece)
    ([EMO_POS, KEY_MAJ], 1, 0, 1, 8, 5, [[NOTE(1), NOTE(2), NOTE(3), NOTE(4)]], (), [BAR]),
    ([EMO_POS, KEY_MAJ], 1, 0, 1, 8, 1000, [LONG], (), [BAR]),
    ([EMO_NEG, KEY_MIN], 1, 0, 2, 8, 1000, [None, [NOTE(1), NOTE(2)]], (1,), [BAR, B(2), BAR]),
    ([EMO_POS, KEY_MAJ], 1, 0, 1, 8, 1000, None, (), []),
    ([EMO_NONE], 1, 1, 1, 5, 1000, [None, [B(2), NOTE(1)], [NOTE(2)]], (),
     [KEY_MIN, KEY_MAJ, NOTE(0), BAR, B(3), NOTE(1), B(1), BAR, BEAT_NEG, B(1), NOTE(3), BAR]),
]
DONE_ROW = 6
ENDS = ['DONE', 'DONE', 'DONE', 'DONE', 'OVERFLOW', 'OVERFLOW', 'DONE', 'DONE']


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Host:
    """One stream of the launch on the host: _LeadSheet is the grammar and the kept-bar rule, step() what a launch does with a RUNNING stream
    that is shown `word` (emo_hip.h, EMO_GRAMMAR_TXL).  keep=False: the stream without its kept bars."""

    def __init__(self, V, row, keep=True, width=WIDTH):
        from emo_disentanger_amd import stage1_inference as s1
        self.s1 = s1
        e2i, self.i2e = vocab(V)
        primer, self.keyed, self.rule, self.mode, max_bars, max_events, kept, self.bad, self.script = row
        self.kept = kept if keep else None
        self.sheet = s1._LeadSheet(e2i, primer, None, max_bars, max_events, self.kept)
        self.plen, self.width = len(primer), width
        self.status, self.feed, self.draws, self.left, self.tok, self.fed = s1.RUNNING, 1, 0, 0, -1, 0
        self.cells = []                                   # (column, word) of every accepted draw

    def word(self):
        return self.script[self.draws] if self.draws < len(self.script) else NOTE(self.draws)

    def state(self):
        s = self.sheet
        return [self.status, len(s.tokens), s.accepted, s.beat, s.bars, s.rejected_in_a_row, self.feed, self.draws]

    def step(self, word):
        s1, s = self.s1, self.sheet
        self.fed += 1
        if self.feed < self.plen:
            self.tok, self.feed = s.tokens[self.feed], self.feed + 1
            return
        if self.left > 0:
            self.tok, self.left = s.tokens[len(s.tokens) - self.left], self.left - 1
            return
        name, took = self.i2e[word], False
        self.draws += 1
        wrong_key = False
        if self.keyed and len(s.tokens) == 1 and self.rule:
            if not name.startswith('Key_'):
                self.status, self.tok = s1.KEY_ERROR, s.tokens[-1]
                return
            wrong_key = not ((self.mode == 1 and name[4:].isupper()) or (self.mode == 2 and name[4:].islower()))
        if not wrong_key:
            before = (len(s.tokens), s.accepted, s.beat, s.bars, s.rejected_in_a_row, s.finished)
            took = s.offer(word, name)
            run = []                                      # the kept bars a chain behind this Bar reaches
            if took and self.kept is not None and name == 'Bar_None':
                j = before[3]
                while j < len(self.kept) and self.kept[j] is not None:
                    run.append(j)
                    j += 1
            if took and (len(s.tokens) > self.width or (s.chained and set(run) & set(self.bad))):
                del s.tokens[before[0]:]                  # the row and the counters as before the draw, which is not counted
                _, s.accepted, s.beat, s.bars, s.rejected_in_a_row, s.finished = before
                s.chained = 0
                self.draws -= 1
                self.status, self.tok = s1.OVERFLOW, s.tokens[-1]
                return
            if took:
                self.cells.append((before[0], int(word)))
        if s.stuck:
            self.status = s1.STUCK
        elif not s.open():
            self.status = s1.DONE
        if self.status == s1.RUNNING and s.accepted == 0:
            self.tok, self.feed = s.tokens[0], 1
        else:
            self.left = s.chained if (took and self.status == s1.RUNNING and self.kept is not None) else 0
            self.tok = s.tokens[-1 - self.left]


def tables_of(rows, keep=True):
    """-> (params, state, seq, kept tables or None) of the rows, packed by stage1_inference.pack_keep; a broken bar gets keep_end = n_keep + 5."""
    from emo_disentanger_amd import stage1_inference as s1
    n = len(rows)
    params, state, seq = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32), np.zeros((n, WIDTH), np.int64)
    for r, (primer, keyed, rule, mode, max_bars, max_events, kept, bad, script) in enumerate(rows):
        seq[r, :len(primer)] = primer
        params[r, :6] = max_bars, max_events, len(primer), keyed, rule, mode
        state[r, [s1.S_STATUS, s1.S_LEN, s1.S_FEED]] = s1.RUNNING, len(primer), 1
    if not keep:
        return params, state, seq, None
    kt, kb, ke, k0, kn = s1.pack_keep([row[6] for row in rows])
    params[:, 6], params[:, 7] = k0, kn
    n_keep = sum(len(b) for row in rows for b in (row[6] or ()) if b is not None)
    broken = [(int(k0[r]) + j) for r, row in enumerate(rows) for j in row[7]]
    return params, state, seq, dict(keep_tok=kt, keep_beg=kb, keep_end=ke, keep_left=np.zeros(n, np.int32), n_keep=n_keep, keep_bar=BAR, broken=broken)


class Rig:
    """Kind TXL over ROWS, common primer prefix 1."""

    def __init__(self, V, seed, keep=True, scores=False, controls=None, guide=None, u_like=None):
        from emo_disentanger_amd import ops, stage1_inference as s1
        self.V, self.ops, self.s1 = V, ops, s1
        self.hosts = [Host(V, row, keep) for row in ROWS]
        self.hosts[DONE_ROW].status = s1.DONE
        _, i2e = vocab(V)
        flags, beat = s1.event_tables(i2e, V)
        params, state, seq, kt = tables_of(ROWS, keep)
        state[DONE_ROW, s1.S_STATUS] = s1.DONE
        U = np.random.RandomState(seed).rand(N_U, N).astype(np.float32)
        for r, c in (u_like or {}).items():
            U[:, r] = U[:, c]
        t = self.t = dict(u_steps=T(U), ev_flags=T(flags), ev_beat=T(beat), params=T(params), state=T(state), seq=T(seq),
                          tok_out=torch.full((N,), -1, dtype=torch.long, device=DEV), running=torch.tensor([N - 1], dtype=torch.int32, device=DEV))
        self.logits = torch.zeros(N, V, device=DEV)
        num = dict(n_rows=N, n_token=V, ld_u=N, temperature=1.2, top_p=0.9, key_temperature=1.1, key_top_p=0.97)
        more = {}
        if kt is not None:
            self.broken = kt.pop('broken')
            num.update(n_keep=kt.pop('n_keep'), keep_bar=kt.pop('keep_bar'))
            more.update({k: T(v) for k, v in kt.items()})
            t['keep_left'] = more.pop('keep_left')
        self.tabs = {}
        if scores:
            self.tabs = ops.draw_score_tables(t['seq'])
        if controls:
            num['n_masks'] = len(controls['tok_mask'])
            more.update({k: T(v.view(np.int32) if k == 'tok_mask' else v) for k, v in controls.items()})
        if guide is not None:
            more.update({k: T(v) for k, v in guide.items()})
        self.args, self.held = ops.GrammarStep(kind=ops.GRAMMAR_TXL), {}
        ops.block_set(self.args, self.held, logits=self.logits, **num, **t, **self.tabs, **more)
        if kt is not None:
            for k in self.broken:                                             # behind block_set's back: it refuses such a range
                more['keep_end'][k] = num['n_keep'] + 5
        self.compared = ('tok_out', 'state', 'seq', 'running') + (('keep_left',) if kt is not None else ())

    def logits_for(self, rs):
        """Row r: noise, no special token or Beat by chance, the word of its next draw boosted."""
        lg = (rs.randn(N, self.V) * 2.0).astype(np.float32)
        lg[:, :NOTE0] = -BOOST
        for r, h in enumerate(self.hosts):
            lg[r, h.word()] = BOOST
        return lg

    def launch(self, lg):
        self.logits.copy_(T(np.ascontiguousarray(lg, dtype=np.float32)))
        self.ops.grammar_step(self.args)
        torch.cuda.synchronize()

    def snap(self):
        return {k: self.t[k].cpu().numpy().copy() for k in self.compared}

    def step_hosts(self):
        for h in self.hosts:
            if h.status == self.s1.RUNNING:
                h.step(h.word())

    def expect(self):
        out = dict(tok_out=np.array([h.tok for h in self.hosts], np.int64), state=np.array([h.state() for h in self.hosts], np.int32),
                   running=np.array([sum(h.status == self.s1.RUNNING for h in self.hosts)], np.int32),
                   keep_left=np.array([h.left for h in self.hosts], np.int32))
        seq = np.zeros((N, WIDTH), np.int64)
        for r, h in enumerate(self.hosts):
            seq[r, :len(h.sheet.tokens)] = h.sheet.tokens
        out['seq'] = seq
        return out

    def check(self, where):
        got, want = self.snap(), self.expect()
        for k in self.compared:
            g, w = got[k], want[k]
            if k == 'seq':                                                    # (beyond LEN a refused chain leaves nothing either: the rows start as zeros)
                assert np.array_equal(g, w), (where, k, [(r, g[r].tolist(), w[r].tolist()) for r in range(N) if not np.array_equal(g[r], w[r])])
            else:
                assert np.array_equal(g, w), (where, k, g.tolist(), w.tolist())


def run_scenario(rig, seed, each=None):
    rs = np.random.RandomState(seed)
    for step in range(LAUNCHES):
        lg = rig.logits_for(rs)
        rig.launch(lg)
        rig.step_hosts()
        rig.check(step)
        if each is not None:
            each(step, lg)
    s1 = rig.s1
    assert [h.status for h in rig.hosts] == [getattr(s1, e) for e in ENDS]
    return rig


def check_the_scenario_was_the_scenario(rig):
    h, s1 = rig.hosts, rig.s1
    assert h[0].sheet.tokens == [EMO_POS, KEY_MAJ, NOTE(0), BAR, B(3), NOTE(1), BAR, B(2), NOTE(1), BAR, NOTE(2), BAR, B(1), NOTE(3), BAR]
    assert h[0].draws == 12 and h[0].sheet.accepted == 9 and h[0].sheet.bars == 5
    assert h[7].sheet.tokens[1:] == h[0].sheet.tokens[1:]
    assert h[1].sheet.tokens == [EMO_NEG, KEY_MIN, NOTE(0), BAR, BAR, B(4), NOTE(5), EOS] and h[1].draws == 6
    assert len(h[2].sheet.tokens) == WIDTH and h[2].sheet.tokens[-1] == BAR and h[2].sheet.bars == 3 and h[2].sheet.accepted == 3
    assert h[3].sheet.tokens == [EMO_POS, KEY_MAJ, BAR, NOTE(1), NOTE(2), NOTE(3)] and h[3].sheet.bars == 1
    assert h[4].state() == [s1.OVERFLOW, 2, 0, 0, 0, 0, 2, 0]
    assert h[5].state() == [s1.OVERFLOW, 4, 2, 2, 1, 0, 2, 2] and h[5].sheet.tokens == [EMO_NEG, KEY_MIN, BAR, B(2)]


@pytest.mark.parametrize('V', [33, 200, 1024])
def test_every_launch_leaves_what_the_host_rule_leaves(V):
    seen = dict(forced_bar_refed=0, chain=0)
    rig = Rig(V, seed=V)

    def each(step, lg):
        h = rig.hosts[0]
        if h.draws == 9 and h.sheet.rejected_in_a_row == 1 and h.sheet.tokens[-1] == BAR and h.left == 0:
            seen['forced_bar_refed'] += int(rig.t['tok_out'][0].item() == BAR and h.sheet.beat == 0)
        seen['chain'] = max(seen['chain'], h.left)

    run_scenario(rig, 3 * V, each)
    check_the_scenario_was_the_scenario(rig)
    assert seen['forced_bar_refed'] == 1 and seen['chain'] == 5, seen
    assert rig.t['tok_out'][DONE_ROW].item() == -1


def controls_for(V):
    """A ban row for rows 0 / 7 and one for row 1 (ids on both sides of a 32-bit word boundary and the last id; no scripted token), per-stream
    temp / top_p, equal in rows 0 / 7."""
    words = (V + 31) // 32
    mask = np.zeros((2, words), np.uint32)
    for m, ids in enumerate(([31, 32, V - 1], [NOTE(7), 32])):
        for v in ids:
            mask[m, v >> 5] |= np.uint32(1 << (v & 31))
    return dict(tok_mask=mask, mask_of=np.array([0, 1, -1, -1, -1, -1, -1, 0], np.int32),
                temp_of=np.array([0.9, 1.4, 1.2, 1.0, 1.2, 0.7, 1.2, 0.9], np.float32),
                top_p_of=np.array([0.8, 0.95, 0.9, 0.9, 1.0, 0.9, 0.9, 0.8], np.float32))


@pytest.mark.parametrize('V', [33, 200])
def test_the_same_with_a_ban_and_per_stream_temp_and_top_p(V):
    rig = run_scenario(Rig(V, seed=V + 1, controls=controls_for(V)), 5 * V)
    check_the_scenario_was_the_scenario(rig)


def guide_tables(s):
    c, g = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    c[[0, 7]], g[[0, 7]] = 0, 7
    sc = np.zeros(N, np.float32)
    sc[[0, 7]] = s
    return dict(guide_cond=c, guide_uncond=g, guide_scale=sc)


def combined(lg, s):
    out = np.array(lg, dtype=np.float32)
    lc, lu = lg[0].astype(np.float32), lg[7].astype(np.float32)
    d = lc - lu
    m = np.float32(s) * d
    out[0] = out[7] = lc + m
    return out


@pytest.mark.parametrize('ctl', [False, True], ids=['plain', 'controls'])
def test_a_guided_pair_with_the_same_kept_bars_is_the_unguided_launch_on_combined_logits(ctl):
    V, s = 200, 1.5
    controls = controls_for(V) if ctl else None
    a = Rig(V, seed=9, controls=controls, guide=guide_tables(s))
    ref = Rig(V, seed=9, controls=controls, u_like={7: 0})
    rs = np.random.RandomState(10)
    for step in range(LAUNCHES):
        lg = a.logits_for(rs)
        lg[7] += (rs.randn(V) * 0.5).astype(np.float32)                      # (the two models differ)
        lg[7, :NOTE0] = lg[0, :NOTE0]
        a.launch(lg)
        ref.launch(combined(lg, s))
        a.step_hosts()
        a.check(step)
        sa, sr = a.snap(), ref.snap()
        for k in a.compared:
            assert np.array_equal(sa[k], sr[k]), (step, k)
        assert np.array_equal(sa['state'][0], sa['state'][7]) and np.array_equal(sa['seq'][0, 1:], sa['seq'][7, 1:]) and sa['keep_left'][0] == sa['keep_left'][7]
    check_the_scenario_was_the_scenario(a)


def ref_scores(row, tok):
    l = row.astype(np.float64)
    mx = l.max()
    lse = mx + np.log(np.exp(l - mx).sum())
    p = np.exp(l - lse)
    return l[tok] - lse, int((l > l[tok]).sum() + (l[:tok] == l[tok]).sum()), lse - float((p * l).sum())


def row_tol(row):
    return ROW_TOL * max(1.0, float(np.spacing(np.float32(np.abs(row).max()))) / ULP16)


def test_only_the_drawn_tokens_cells_are_written_the_kept_cells_keep_the_pre_fill():
    V = 200
    rig = Rig(V, seed=4, scores=True)
    rows = {}

    def each(step, lg):
        for r, h in enumerate(rig.hosts):
            for c, w in h.cells:
                rows.setdefault((r, c), (lg[r].copy(), w))

    run_scenario(rig, 6, each)
    lp, rk, en = (rig.tabs[k].cpu().numpy() for k in TABLES)
    cells = np.zeros((N, WIDTH), bool)
    for (r, c), (row, w) in rows.items():
        cells[r, c] = True
        logp, rank, ent = ref_scores(row, w)
        assert rk[r, c] == rank and abs(float(lp[r, c]) - logp) <= row_tol(row) and abs(float(en[r, c]) - ent) <= row_tol(row), (r, c)
    assert np.array_equal(rk >= 0, cells) and np.array_equal(~np.isnan(lp), cells) and np.array_equal(~np.isnan(en), cells)
    # row 0: its chain lies at columns 7 .. 11 behind the Bar drawn at 6; row 2: 43 kept tokens and the closing Bar behind column 3
    assert cells[0, 6] and not cells[0, 7:12].any() and cells[0, 12] and cells[2, 3] and not cells[2, 4:].any() and int(cells.sum()) == sum(len(h.cells) for h in rig.hosts)
    from emo_disentanger_amd import scoring
    ids = rig.hosts[0].sheet.tokens
    rec = scoring.draw_record(ids, lp[0, :len(ids)], rk[0, :len(ids)], en[0, :len(ids)])
    assert rec['n_tokens'] == 15 and rec['n_scored'] == rig.hosts[0].sheet.accepted == 9             # draw_record counts no kept cell as a draw


def test_with_the_tables_null_kind_txl_leaves_what_it_leaves_without_the_fields():
    V = 200
    a = Rig(V, seed=21, keep=False, scores=True)
    b = Rig(V, seed=21, keep=False, scores=True)
    assert a.args.keep_tok is None and a.args.keep_beg is None and a.args.keep_end is None and a.args.keep_left is None and a.args.keep_bar == 0
    rs = np.random.RandomState(22)
    for step in range(LAUNCHES):
        lg = a.logits_for(rs)
        a.launch(lg)
        a.step_hosts()
        a.check(step)                                                         # the host rule without keep: generate_plain_xl_batch's grammar
        b.logits.copy_(T(lg))
        t = b.t                                                               # a fresh block per call, built by the wrapper, which knows none of the fields
        a.ops.txl_grammar_step(b.logits, 1.2, 0.9, 1.1, 0.97, t['u_steps'], t['ev_flags'], t['ev_beat'], t['params'], t['state'], t['seq'], t['tok_out'],
                               t['running'], **b.tabs)
        torch.cuda.synchronize()
        sa, sb = a.snap(), b.snap()
        for k in a.compared:
            assert np.array_equal(sa[k], sb[k]), (step, k)
    for k in TABLES:
        assert np.array_equal(a.tabs[k].view(torch.int32).cpu().numpy(), b.tabs[k].view(torch.int32).cpu().numpy()), k
    assert a.hosts[0].sheet.bars >= 2 and a.hosts[4].status == a.s1.RUNNING                # (no chain, no overflow: the rows draw on)


# ------------------------------------------------------------------------------------------------ kind TXL_QUEUE
# (job 2: row 2 with a bar more to go, so that its kept run does not end the piece in the launch that writes it and has to be fed)
JOBS = [ROWS[0], ROWS[1], ROWS[2][:4] + (4,) + ROWS[2][5:], ROWS[3], ROWS[4], ROWS[5], ROWS[7]]
SLOTS, MEM_ROWS = 3, 30


class QueueRig:
    """Seven jobs through three slots.  The model step is stood in for by what it does to the launch's arrays: every row's length goes up by 1."""

    def __init__(self, V, seed, keep=True, wrapper=False):
        from emo_disentanger_amd import ops, stage1_inference as s1
        self.V, self.ops, self.s1, self.wrapper = V, ops, s1, wrapper
        n = len(JOBS)
        self.hosts = [Host(V, row, keep) for row in JOBS]
        _, i2e = vocab(V)
        flags, beat = s1.event_tables(i2e, V)
        params, state, seq, kt = tables_of(JOBS, keep)
        t = self.t = dict(u_steps=T(np.random.RandomState(seed).rand(N_U, n).astype(np.float32)), ev_flags=T(flags), ev_beat=T(beat), params=T(params),
                          state=T(state), seq=T(seq), tok_out=torch.zeros(SLOTS, dtype=torch.long, device=DEV),
                          running=torch.tensor([n], dtype=torch.int32, device=DEV), slot_job=torch.full((SLOTS,), -1, dtype=torch.int32, device=DEV),
                          queue_head=torch.zeros(1, dtype=torch.int32, device=DEV), mem_lens=torch.zeros(SLOTS, dtype=torch.long, device=DEV),
                          job_steps=torch.full((n,), -7, dtype=torch.int32, device=DEV))
        self.logits = torch.zeros(SLOTS, V, device=DEV)
        num = dict(n_rows=SLOTS, n_token=V, ld_u=n, n_jobs=n, mem_rows=MEM_ROWS, temperature=1.2, top_p=0.9, key_temperature=1.1, key_top_p=0.97)
        more = {}
        if kt is not None:
            broken = kt.pop('broken')
            num.update(n_keep=kt.pop('n_keep'), keep_bar=kt.pop('keep_bar'))
            more.update({k: T(v) for k, v in kt.items()})
            t['keep_left'] = more.pop('keep_left')
        self.args, self.held = ops.GrammarStep(kind=ops.GRAMMAR_TXL_QUEUE), {}
        ops.block_set(self.args, self.held, logits=self.logits, **num, **t, **more)
        if kt is not None:
            for k in broken:
                more['keep_end'][k] = num['n_keep'] + 5
        self.book, self.ended_at = [-1] * SLOTS, {}

    def launch(self, rs, where):
        s1, t = self.s1, self.t
        lens = t['mem_lens'].cpu().tolist()
        lg = (rs.randn(SLOTS, self.V) * 2.0).astype(np.float32)
        lg[:, :NOTE0] = -BOOST
        for b, j in enumerate(self.book):
            if j >= 0:
                lg[b, self.hosts[j].word()] = BOOST
        self.logits.copy_(T(lg))
        if self.wrapper:
            self.ops.txl_queue_step(self.logits, 1.2, 0.9, 1.1, 0.97, t['u_steps'], t['ev_flags'], t['ev_beat'], t['params'], t['state'], t['seq'],
                                    t['tok_out'], t['running'], t['slot_job'], t['queue_head'], t['mem_lens'], MEM_ROWS, job_steps=t['job_steps'])
        else:
            self.ops.grammar_step(self.args)
        torch.cuda.synchronize()
        st, sq, tk, sj = t['state'].cpu().numpy(), t['seq'].cpu().numpy(), t['tok_out'].cpu().tolist(), t['slot_job'].cpu().tolist()
        left = t['keep_left'].cpu().tolist() if 'keep_left' in t else None
        freed = []
        for b, j in enumerate(self.book):
            if j < 0:
                freed.append(b)
                continue
            h = self.hosts[j]
            if lens[b] >= MEM_ROWS:
                h.status = s1.MEM_FULL
            else:
                h.step(h.word())
            assert st[j].tolist() == h.state(), (where, b, j, st[j].tolist(), h.state())
            assert sq[j, :len(h.sheet.tokens)].tolist() == h.sheet.tokens and not sq[j, len(h.sheet.tokens):].any(), (where, b, j)
            if h.status == s1.RUNNING:
                assert sj[b] == j and tk[b] == h.tok and (left is None or left[j] == h.left), (where, b, j)
            else:
                if h.status != s1.MEM_FULL:
                    h.fed -= 1                                                 # (the output of the launch that ends a job is not fed for it)
                self.ended_at[j] = lens[b]
                freed.append(b)
        for b in freed:
            self.book[b] = sj[b]
            if sj[b] >= 0:
                h = self.hosts[sj[b]]
                assert tk[b] == h.sheet.tokens[0] and st[sj[b], s1.S_FEED] == 1
                h.feed, h.fed = 1, 1
        assert int(t['running'].item()) == sum(h.status == s1.RUNNING for h in self.hosts), where
        t['mem_lens'].add_(1)                                                  # the model step behind the launch

    def run(self, seed):
        rs = np.random.RandomState(seed)
        for where in range(120):
            self.launch(rs, where)
            if all(h.status != self.s1.RUNNING for h in self.hosts):
                return self
        raise AssertionError('the queue did not drain')


@pytest.mark.parametrize('V', [33, 200])
def test_queue_jobs_equal_their_lock_step_runs_and_job_steps_counts_the_kept_tokens(V):
    q = QueueRig(V, seed=V).run(V + 2)
    s1 = q.s1
    lock = run_scenario(Rig(V, seed=V), 3 * V)                               # the lock-step launch over the same rows
    for j, r in enumerate([0, 1, 2, 3, 4, 5, 7]):
        if j == 2:
            continue
        assert q.hosts[j].sheet.tokens == lock.hosts[r].sheet.tokens and q.hosts[j].status == lock.hosts[r].status, j
    # job 2: 4 tokens and a kept run of 44 do not fit 30 rows of memory: the chain is in its row, the feed stops at the bound
    assert q.hosts[2].status == s1.MEM_FULL and len(q.hosts[2].sheet.tokens) == WIDTH and q.hosts[2].fed == MEM_ROWS
    steps = q.t['job_steps'].cpu().tolist()
    assert steps == [q.ended_at[j] for j in range(len(JOBS))]
    # a job's launches are the tokens it was fed: the primer (twice where it was fed again), one per draw but the last (accepted or not: a
    # rejection feeds an input again), the kept ones
    h = q.hosts[0]
    assert steps[0] == h.fed == 1 + (h.draws - 1) + 5 == 17 and steps[1] == q.hosts[1].fed == 3 + 2 + (6 - 1) + 1 and steps[2] == MEM_ROWS
    assert sorted(q.ended_at) == list(range(len(JOBS))) and q.t['slot_job'].cpu().tolist() == [-1] * SLOTS


def test_with_the_tables_null_kind_txl_queue_leaves_what_it_leaves_without_the_fields():
    V = 200
    a = QueueRig(V, seed=5, keep=False)
    b = QueueRig(V, seed=5, keep=False, wrapper=True)
    assert a.args.keep_tok is None and a.args.keep_left is None
    ra, rb = np.random.RandomState(6), np.random.RandomState(6)
    for where in range(40):                                                    # (without kept bars the jobs draw on: the rows fill up to MEM_FULL)
        a.launch(ra, where)
        b.launch(rb, where)
        for k in ('state', 'seq', 'running', 'queue_head', 'job_steps'):        # per job (which of the slots freed in one launch gets which job is not specified)
            assert torch.equal(a.t[k], b.t[k]), (where, k)
        assert sorted(a.t['slot_job'].tolist()) == sorted(b.t['slot_job'].tolist()) and sorted(a.t['mem_lens'].tolist()) == sorted(b.t['mem_lens'].tolist()), where
    assert any(h.status == a.s1.MEM_FULL for h in a.hosts)
