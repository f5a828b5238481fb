"""GPU: classifier-free guidance in the stage-1 device draw (emo_grammar_step, kind TXL: guide_cond / guide_uncond / guide_scale), kernel level, on
synthetic fp32 logits and a small synthetic grammar.  Six rows: the pairs (0, 3) with scale 1.5 and (1, 4) with scale 0 or 0.75, stream 2
without guidance and stream 5 finished before the first launch, driven through a key draw under the key rule that is rejected and one that is
accepted, primer feeds beyond the common prefix, a PAD draw, the re-feed of a whole primer while nothing is accepted, Beat-heavy launches
(a Beat that goes back re-feeds the previous input), a Bar and the closing EOS:
  - after EVERY launch the guided block leaves, bit for bit, what a block WITHOUT the fields leaves on logits combined on the host in NumPy
    float32, lc + s * (lc - lu) as three rounded operations written into both rows of a pair, the follower's uniform column set to its leader's;
  - the same with a ban and per-stream temp / top_p on top; the draw of a pair runs under the controls of its conditioned row;
  - scale 0 is the conditioned row itself;
  - the recorded scores are each row's own model's: the leader's from the conditioned row, the follower's from the unconditioned row, for the
    same tokens, held to float64 as tests/test_gpu_draw_scores.py holds them;
  - with the three fields NULL the block leaves word for word what ops.txl_grammar_step leaves."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N = 6
S_STATUS, S_LEN, S_ACCEPTED, S_BEAT, S_BARS, S_FAILED, S_FEED, S_DRAWS = range(8)
EMO_POS, EMO_NEG, EMO_NONE, KEY_MAJ, KEY_MIN, BAR, PAD, EOS, BEAT0, N_BEATS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 16
EV_BEAT, EV_BAR, EV_PAD, EV_EOS, EV_KEY, EV_MAJOR, EV_MINOR = 1, 2, 4, 8, 16, 32, 64
RUNNING, DONE = 0, 1
TABLES = ('tok_logp', 'tok_rank', 'tok_entropy')
COMPARED = ('tok_out', 'state', 'seq', 'running')
ROW_TOL = 1e-5                       # tests/test_gpu_draw_scores.py: absolute, per row, at the logit scale randn x 3 (|l| < 16) ...
ULP16 = float(np.spacing(np.float32(15.99)))
BOOST = 60.0                         # a logit that wins its launch in every row, combined or not
STEPS = 19
SCALE_B = {33: 0.0, 200: 0.75, 1024: 0.0}


def row_tol(row):
    """... scaled, as there, by the ulp of the row's largest |logit| where that is above the scale ROW_TOL was derived at."""
    return ROW_TOL * max(1.0, float(np.spacing(np.float32(np.abs(row).max()))) / ULP16)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pairs(sb):
    return {0: (0, 3, 1.5), 3: (0, 3, 1.5), 1: (1, 4, sb), 4: (1, 4, sb)}          # stream -> (cond, uncond, scale)


def guide_tables(sb):
    p = pairs(sb)
    return dict(guide_cond=np.array([p[r][0] if r in p else -1 for r in range(N)], np.int32),
                guide_uncond=np.array([p[r][1] if r in p else -1 for r in range(N)], np.int32),
                guide_scale=np.array([p[r][2] if r in p else 0.0 for r in range(N)], np.float32))


def combined(logits, sb):
    """The host restatement: NumPy float32, three separately rounded operations, written into both rows of every pair."""
    out = np.array(logits, dtype=np.float32)
    for r, (c, g, s) in pairs(sb).items():
        lc, lu = logits[c].astype(np.float32), logits[g].astype(np.float32)
        d = lc - lu
        m = np.float32(s) * d
        out[r] = lc + m
    assert out.dtype == np.float32
    return out


class Rig:
    """Kind TXL, common primer prefix 1.  Pair A (rows 0 / 3): a one-token primer (the tag; the follower's is Emotion_None), keyed, under the
    key rule with the LEADER's mode in both rows.  Pair B (rows 1 / 4): a three-token primer of which two are still to be fed.  Row 2: a
    keyed stream without the rule and without guidance.  Row 5: DONE."""

    def __init__(self, V, seed, width=48, n_u=64):
        self.V, self.width = V, width
        rs = np.random.RandomState(seed)
        self.flags, self.beat = np.zeros(V, np.int32), np.zeros(V, np.int32)
        self.flags[BEAT0:BEAT0 + N_BEATS], self.beat[BEAT0:BEAT0 + N_BEATS] = EV_BEAT, np.arange(N_BEATS)
        self.flags[[KEY_MAJ, KEY_MIN, BAR, PAD, EOS]] = EV_KEY | EV_MAJOR, EV_KEY | EV_MINOR, EV_BAR, EV_PAD, EV_EOS
        self.U = rs.rand(n_u, N).astype(np.float32)
        self.seq = np.zeros((N, width), np.int64)
        primers = [[EMO_POS], [EMO_NEG, KEY_MIN, BAR], [EMO_NEG], [EMO_NONE], [EMO_NONE, KEY_MIN, BAR], [EMO_POS, KEY_MAJ]]
        self.params, self.state = np.zeros((N, 8), np.int32), np.zeros((N, 8), np.int32)
        for r, p in enumerate(primers):
            self.seq[r, :len(p)] = p
            self.params[r, :6] = 8, 1000, len(p), 1, r in (0, 3), 1 if r in (0, 3) else 2      # MAX_BARS, MAX_EVENTS, PRIMER_LEN, KEYED, KEY_RULE, EMO_MODE
            self.state[r, [S_STATUS, S_LEN, S_BARS, S_FEED]] = RUNNING, len(p), len(p) == 3, 1
        self.state[5, S_STATUS] = DONE

    def build(self, guide=None, scores=False, controls=None):
        from emo_disentanger_amd import ops
        t = self.t = dict(u_steps=T(self.U), ev_flags=T(self.flags), ev_beat=T(self.beat), params=T(self.params), state=T(self.state), seq=T(self.seq),
                          tok_out=torch.full((N,), -1, dtype=torch.long, device=DEV), running=torch.tensor([N - 1], dtype=torch.int32, device=DEV))
        self.logits = torch.zeros(N, self.V, device=DEV)
        num = dict(n_rows=N, n_token=self.V, ld_u=N, temperature=1.2, top_p=0.9, key_temperature=1.1, key_top_p=0.97)
        self.tabs = {}
        if scores:
            self.tabs = {k: torch.full((N, self.width), -1 if k == 'tok_rank' else float('nan'), device=DEV,
                                       dtype=torch.int32 if k == 'tok_rank' else torch.float32) for k in TABLES}
        more = {}
        if controls:
            num['n_masks'] = len(controls['tok_mask'])
            more = {k: T(v.view(np.int32) if k == 'tok_mask' else v) for k, v in controls.items()}
        if guide is not None:
            more.update({k: T(v) for k, v in guide_tables(guide).items()})
        self.args, self.held = ops.GrammarStep(kind=ops.GRAMMAR_TXL), {}
        ops.block_set(self.args, self.held, logits=self.logits, **num, **t, **self.tabs, **more)
        return self

    def launch(self, logits):
        from emo_disentanger_amd import ops
        self.logits.copy_(T(np.ascontiguousarray(logits, dtype=np.float32)))
        ops.grammar_step(self.args)
        torch.cuda.synchronize()

    def snap(self):
        return {k: self.t[k].cpu().numpy().copy() for k in COMPARED}


HEAVY = (3, 4, 5, 6, 7, 11, 12)


def schedule(rig, rs, step):
    """The logits of launch `step`.  0: a minor key (pair A, mode major under the rule: rejected, nothing accepted yet, the primer again; row 2
    accepts it).  1: a major key (pair A accepts).  2: PAD (pair B's first draw: rejected with nothing accepted, its three primer tokens are
    fed again over the next launches; the others feed their previous input again).  3 - 7, 11, 12: Beat-heavy (a Beat that goes back is
    rejected).  8, 9, 13 - 16: any unmarked token, the rows far apart.  10: Bar.  17: EOS.  18: finished streams."""
    heavy = step in HEAVY
    logits = (rs.randn(N, rig.V) * (0.5 if heavy else 2.0)).astype(np.float32)
    # (Beats: likely and alike in every row, so that none dominates a combined row and runs a stream into STUCK; absent elsewhere)
    logits[:, BEAT0:BEAT0 + N_BEATS] = (7.0 + 0.5 * rs.randn(N_BEATS)).astype(np.float32) if heavy else -BOOST
    for tok, at in ((KEY_MIN, 0), (KEY_MAJ, 1), (PAD, 2), (BAR, 10), (EOS, 17)):
        logits[:, tok] = BOOST if step == at else -BOOST         # (never drawn by chance: every stream follows the schedule)
    return logits


def controls_for(V, follower=None):
    """A ban row per pair (ids on both sides of a 32-bit word boundary, a Beat and the last id among them; no scheduled token), per-stream temp /
    top_p, equal within a pair; stream 2 has no ban.  follower: other controls in the followers' rows 3 / 4 (mask, temp, top_p)."""
    words = (V + 31) // 32
    mask = np.zeros((2, words), np.uint32)
    for m, ids in enumerate(([BEAT0, 31, 32, V - 1], [BEAT0 + 1, 0, 32])):
        for v in ids:
            mask[m, v >> 5] |= np.uint32(1 << (v & 31))
    out = dict(tok_mask=mask, mask_of=np.array([0, 1, -1, 0, 1, -1], np.int32), temp_of=np.array([0.9, 1.4, 1.2, 0.9, 1.4, 1.0], np.float32),
               top_p_of=np.array([0.8, 0.95, 0.9, 0.8, 0.95, 0.9], np.float32))
    if follower is not None:
        for r in (3, 4):
            out['mask_of'][r], out['temp_of'][r], out['top_p_of'][r] = follower
    return out


def reference(V, seed, sb, controls, scores=False):
    """The block without the fields: both rows of a pair read the leader's uniform column."""
    ref = Rig(V, seed)
    for r, (c, g, s) in pairs(sb).items():
        ref.U[:, r] = ref.U[:, c]
    return ref.build(controls=controls, scores=scores)


@pytest.mark.parametrize('ctl', [False, True], ids=['plain', 'controls'])
@pytest.mark.parametrize('V', [33, 200, 1024])
def test_a_guided_launch_is_the_unguided_launch_on_logits_combined_on_the_host(V, ctl):
    sb = SCALE_B[V]
    controls = controls_for(V) if ctl else None
    a = Rig(V, seed=V).build(guide=sb, controls=controls)
    ref = reference(V, V, sb, controls)
    zero = None
    if sb == 0.0:                                                              # scale 0: both rows hold the CONDITIONED logits, nothing is combined
        zero = Rig(V, seed=V)
        zero.U[:, 4] = zero.U[:, 1]
        zero.build(controls=controls)
    rs = np.random.RandomState(7 * V + ctl)
    seen = dict(key_rejected=0, key_accepted=0, pad=0, refeed=0, beat_rejected=0, feeding=0)
    for step in range(STEPS):
        logits = schedule(a, rs, step)
        s0 = a.t['state'].cpu().numpy().copy()
        a.launch(logits)
        comb = combined(logits, sb)
        if sb == 0.0:
            assert np.array_equal(comb[1].view(np.int32), logits[1].view(np.int32)) and np.array_equal(comb[4].view(np.int32), logits[1].view(np.int32))
        ref.launch(comb)
        sa, sr = a.snap(), ref.snap()
        for k in COMPARED:
            assert np.array_equal(sa[k], sr[k]), (step, k, sa[k].tolist(), sr[k].tolist())
        if zero is not None:
            plain = logits.copy()
            plain[4] = logits[1]
            zero.launch(plain)
            sz = zero.snap()
            for k in ('tok_out', 'state', 'seq'):
                assert np.array_equal(sa[k][[1, 4]], sz[k][[1, 4]]), (step, k)
        # the pair invariant: the follower stays word for word with its leader, its first primer token apart
        for c, g in ((0, 3), (1, 4)):
            assert np.array_equal(sa['state'][c], sa['state'][g]) and np.array_equal(sa['seq'][c, 1:], sa['seq'][g, 1:]), (step, c, g)
            assert sa['tok_out'][c] == sa['tok_out'][g] or (sa['tok_out'][c], sa['tok_out'][g]) in ((EMO_POS, EMO_NONE), (EMO_NEG, EMO_NONE)), (step, c, g)
        assert sa['seq'][:, 0].tolist() == [EMO_POS, EMO_NEG, EMO_NEG, EMO_NONE, EMO_NONE, EMO_POS]
        assert np.array_equal(sa['state'][5], a.state[5]) and sa['tok_out'][5] == -1                   # the finished row is left alone
        s1 = sa['state']
        drew = s1[:, S_DRAWS] > s0[:, S_DRAWS]
        rejected = drew & (s1[:, S_LEN] == s0[:, S_LEN]) & (s1[:, S_STATUS] == RUNNING)
        seen['key_rejected'] += int(step == 0 and rejected[0] and rejected[3] and s1[0, S_ACCEPTED] == 0 and sa['tok_out'][3] == EMO_NONE)
        seen['key_accepted'] += int(step == 1 and sa['seq'][0, 1] == KEY_MAJ and sa['seq'][3, 1] == KEY_MAJ and s1[3, S_ACCEPTED] == 1)
        seen['pad'] += int(step == 2 and rejected[[0, 1, 2, 3, 4]].all())
        seen['refeed'] += int(step == 2 and s1[1, S_FEED] == 1 and s1[4, S_FEED] == 1 and sa['tok_out'][1] == EMO_NEG and sa['tok_out'][4] == EMO_NONE)
        seen['beat_rejected'] += int((rejected & (s1[:, S_FAILED] > s0[:, S_FAILED]))[[0, 1, 3, 4]].sum())
        seen['feeding'] += int(((s1[:, S_FEED] > s0[:, S_FEED]) & ~drew)[[1, 4]].sum())
    st = a.t['state'].cpu().numpy()
    assert (st[:, S_STATUS] == DONE).all() and int(a.t['running'].item()) == 0
    assert seen['key_rejected'] == 1 and seen['key_accepted'] == 1 and seen['pad'] == 1 and seen['refeed'] == 1, seen
    assert seen['beat_rejected'] >= 4 and seen['feeding'] == 8, seen           # pair B: two primer tokens beyond the prefix, twice, in both rows
    seq = a.t['seq'].cpu().numpy()
    assert (seq[np.arange(N - 1), st[:N - 1, S_LEN] - 1] == EOS).all() and st[0, S_BARS] == 1 and st[1, S_BARS] == 2
    if ctl:
        assert not set(seq[0, 1:st[0, S_LEN]].tolist()) & {BEAT0, 31, 32, V - 1}
        assert not set(seq[1, 3:st[1, S_LEN]].tolist()) & {BEAT0 + 1, 0, 32}
    # the guidance moved a draw: the leader's ids are not those of its conditioned row alone; the unguided stream's are
    alone = Rig(V, seed=V).build(controls=controls)
    rs = np.random.RandomState(7 * V + ctl)
    for step in range(STEPS):
        alone.launch(schedule(alone, rs, step))
    other = alone.t['seq'].cpu().numpy()
    assert not np.array_equal(other[0], seq[0]) and np.array_equal(other[2], seq[2])
    if sb == 0.0:
        assert np.array_equal(other[1], seq[1])


def test_the_draw_of_a_pair_runs_under_the_controls_of_its_conditioned_row():
    # the followers' rows hold other controls (no ban, temp 1.0, top_p 0.5): the pair still draws under the leader's, both rows alike
    V, sb = 200, 0.75
    a = Rig(V, seed=5).build(guide=sb, controls=controls_for(V, follower=(-1, 1.0, 0.5)))
    ref = reference(V, 5, sb, controls_for(V))
    rs = np.random.RandomState(6)
    for step in range(STEPS):
        logits = schedule(a, rs, step)
        a.launch(logits)
        ref.launch(combined(logits, sb))
        sa, sr = a.snap(), ref.snap()
        for k in COMPARED:
            assert np.array_equal(sa[k], sr[k]), (step, k)
    assert (a.t['state'].cpu().numpy()[:, S_STATUS] == DONE).all()


def ref_scores(row, tok):
    l = row.astype(np.float64)
    mx = l.max()
    lse = mx + np.log(np.exp(l - mx).sum())
    p = np.exp(l - lse)
    return l[tok] - lse, int((l > l[tok]).sum() + (l[:tok] == l[tok]).sum()), lse - float((p * l).sum())


def test_the_scores_of_a_pair_are_each_rows_own_models_for_the_same_tokens():
    V, sb = 200, 0.75
    a = Rig(V, seed=11).build(guide=sb, scores=True)
    rs = np.random.RandomState(12)
    hits = []
    for step in range(STEPS):
        logits = schedule(a, rs, step)
        s0 = a.t['state'].cpu().numpy().copy()
        a.launch(logits)
        s1, seq = a.t['state'].cpu().numpy(), a.t['seq'].cpu().numpy()
        for r in range(N):
            if s1[r, S_ACCEPTED] > s0[r, S_ACCEPTED]:
                hits.append((r, int(s0[r, S_LEN]), int(seq[r, s0[r, S_LEN]]), logits[r].copy()))
    assert len(hits) >= 5 * (N - 1)
    lp, rk, en = (a.tabs[k].cpu().numpy() for k in TABLES)
    cells = np.zeros((N, a.width), bool)
    for r, c, tok, row in hits:
        cells[r, c] = True
        logp, rank, ent = ref_scores(row, tok)                                  # the stream's OWN row, as the model wrote it
        assert rk[r, c] == rank, (r, c)
        assert abs(float(lp[r, c]) - logp) <= row_tol(row) and abs(float(en[r, c]) - ent) <= row_tol(row), (r, c)
    assert np.array_equal(rk >= 0, cells) and np.array_equal(~np.isnan(lp), cells) and np.array_equal(~np.isnan(en), cells)
    assert np.array_equal(cells[0], cells[3]) and np.array_equal(cells[1], cells[4]) and not cells[5].any() and not cells[:, 0].any()
    # the device's own row scorer on the same rows
    from emo_disentanger_amd import ops
    ts = ops.token_scores(T(np.stack([h[3] for h in hits])), torch.tensor([h[2] for h in hits], device=DEV), -100, want=('rank', 'entropy'))
    nll, rank = ts['nll'].cpu().numpy(), ts['rank'].cpu().numpy()
    for i, (r, c, tok, row) in enumerate(hits):
        assert rk[r, c] == rank[i] and abs(float(lp[r, c]) + float(nll[i])) <= 2 * row_tol(row), (r, c)
    # the follower's figures are another model's for the same token: they differ from the leader's
    both = cells[0]
    assert not np.array_equal(lp[0][both], lp[3][both]) and not np.array_equal(rk[0][both], rk[3][both])


def test_the_unguided_scores_of_a_row_are_what_the_guided_launch_records_for_it():
    # per recorded draw of the guided launch, an unguided one-stream launch on the row's own logits that is made to draw the same token (every
    # other one banned: a ban reaches the draw alone) records the same cell, bit for bit, for the leader's and for the follower's row
    V, sb = 200, 0.75
    a = Rig(V, seed=31).build(guide=sb, scores=True)
    rs = np.random.RandomState(32)
    recorded = []
    for step in range(STEPS):
        logits = schedule(a, rs, step)
        s0 = a.t['state'].cpu().numpy().copy()
        a.launch(logits)
        s1, seq = a.t['state'].cpu().numpy(), a.t['seq'].cpu().numpy()
        for r in range(N):
            if s1[r, S_ACCEPTED] > s0[r, S_ACCEPTED]:
                recorded.append((r, int(s0[r, S_LEN]), int(seq[r, s0[r, S_LEN]]), logits[r].copy()))
    from emo_disentanger_amd import ops
    lp, rk, en = (a.tabs[k] for k in TABLES)
    words = (V + 31) // 32
    for r, c, tok, row in recorded[:12] + recorded[-4:]:
        mask = np.full((1, words), 0xFFFFFFFF, np.uint32)
        mask[0, tok >> 5] &= np.uint32(~(1 << (tok & 31)) & 0xFFFFFFFF)
        seq1 = np.zeros((1, a.width), np.int64)
        seq1[0, :c] = 24
        state1, params1 = np.zeros((1, 8), np.int32), np.zeros((1, 8), np.int32)
        params1[0, :3] = 100, 1000, c                                           # (not keyed: the grammar takes any token but a Beat going back)
        state1[0, [S_LEN, S_FEED, S_ACCEPTED]] = c, c, 1
        tabs = {k: torch.full((1, a.width), -1 if k == 'tok_rank' else float('nan'), device=DEV, dtype=torch.int32 if k == 'tok_rank' else torch.float32)
                for k in TABLES}
        args, held = ops.GrammarStep(kind=ops.GRAMMAR_TXL), {}
        ops.block_set(args, held, n_rows=1, n_token=V, ld_u=1, temperature=1.2, top_p=0.9, key_temperature=1.1, key_top_p=0.97, n_masks=1,
                      logits=T(row[None]), u_steps=T(np.full((1, 1), 0.5, np.float32)), ev_flags=a.t['ev_flags'], ev_beat=a.t['ev_beat'], params=T(params1),
                      state=T(state1), seq=T(seq1), tok_out=torch.zeros(1, dtype=torch.long, device=DEV),
                      running=torch.ones(1, dtype=torch.int32, device=DEV), tok_mask=T(mask.view(np.int32)), mask_of=T(np.zeros(1, np.int32)), **tabs)
        ops.grammar_step(args)
        assert int(held['seq'][0, c].item()) == tok, (r, c)
        for k, t in zip(TABLES, (lp, rk, en)):
            assert torch.equal(tabs[k][0, c].view(torch.int32), t[r, c].view(torch.int32)), (r, c, k)


def test_with_the_three_fields_null_the_block_leaves_what_the_one_shot_step_leaves():
    from emo_disentanger_amd import ops
    V = 200
    a = Rig(V, seed=21).build(scores=True)
    b = Rig(V, seed=21).build(scores=True)
    assert a.args.guide_cond is None and a.args.guide_uncond is None and a.args.guide_scale is None
    rs = np.random.RandomState(22)
    for step in range(STEPS):
        logits = schedule(a, rs, step)
        a.launch(logits)
        b.logits.copy_(T(logits))
        t = b.t                                                                 # a fresh block per call, built by the wrapper, its guidance arguments left out
        ops.txl_grammar_step(b.logits, 1.2, 0.9, 1.1, 0.97, t['u_steps'], t['ev_flags'], t['ev_beat'], t['params'], t['state'], t['seq'], t['tok_out'],
                             t['running'], **b.tabs)
        torch.cuda.synchronize()
        sa, sb = a.snap(), b.snap()
        for k in COMPARED:
            assert np.array_equal(sa[k], sb[k]), (step, k)
    for k in TABLES:
        assert np.array_equal(a.tabs[k].view(torch.int32).cpu().numpy(), b.tabs[k].view(torch.int32).cpu().numpy()), k
    assert int((a.tabs['tok_rank'] >= 0).sum().item()) >= 5 * (N - 1) and (a.t['state'].cpu().numpy()[:, S_STATUS] == DONE).all()
