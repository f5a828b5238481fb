"""GPU: classifier-free guidance in the stage-2 device draw (emo_grammar_step, kind ACC: guide_cond / guide_uncond / guide_scale), kernel level, on
synthetic fp32 logits and a small synthetic grammar.  Five streams: the pairs (0, 1) with scale 1.5 and (3, 4) with scale 0, and stream 2 without
guidance between them, driven through primer feeds, Beat-heavy launches (in-launch redraws), an injected lead-sheet bar and the closing EOS:
  - after EVERY launch the guided block leaves, bit for bit, what a block WITHOUT the fields leaves on logits combined on the host in NumPy
    float32, lc + s * (lc - lu) written into both rows of a pair, the follower's uniform column set to its leader's;
  - the same with a ban and per-stream temp / top_p on top;
  - scale 0 is the conditioned row itself;
  - the recorded scores are each row's own model's: the leader's from the conditioned row, the follower's from the unconditioned row, for the
    same tokens, held to emo_token_scores and float64 as tests/test_gpu_draw_scores.py holds them;
  - with the three fields NULL the block leaves word for word what ops.acc_grammar_step leaves."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
N = 5
PAIRS = {0: (0, 1, 1.5), 1: (0, 1, 1.5), 3: (3, 4, 0.0), 4: (3, 4, 0.0)}           # stream -> (cond, uncond, scale)
COND = np.array([PAIRS[r][0] if r in PAIRS else -1 for r in range(N)], np.int32)
UNCOND = np.array([PAIRS[r][1] if r in PAIRS else -1 for r in range(N)], np.int32)
SCALE = np.array([PAIRS[r][2] if r in PAIRS else 0.0 for r in range(N)], np.float32)
S_STATUS, S_LEN, S_CONSUMED, S_BARS, S_DRAWS, S_ACCEPTED = 0, 1, 2, 3, 6, 7
TRACK_LS, TRACK_FULL, BEAT0, N_BEATS, PAD, EOS = 5, 6, 8, 16, 24, 25
TABLES = ('tok_logp', 'tok_rank', 'tok_entropy')
COMPARED = ('tok_out', 'seg_out', 'state', 'seq', 'segs', 'running')
ROW_TOL = 1e-5                       # tests/test_gpu_draw_scores.py: absolute, per row, at the logit scale randn x 3 (|l| < 16) ...
ULP16 = float(np.spacing(np.float32(15.99)))
BOOST = 60.0                         # a logit that wins its launch in every row, combined or not


def row_tol(row):
    """... scaled, as there, by the ulp of the row's largest |logit| where that is above the scale ROW_TOL was derived at."""
    return ROW_TOL * max(1.0, float(np.spacing(np.float32(np.abs(row).max()))) / ULP16)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def combined(logits):
    """The host restatement: NumPy float32, three rounded operations, written into both rows of every pair."""
    out = np.array(logits, dtype=np.float32)
    for r, (c, g, s) in PAIRS.items():
        lc, lu = logits[c].astype(np.float32), logits[g].astype(np.float32)
        out[r] = lc + np.float32(s) * (lc - lu)
    assert out.dtype == np.float32
    return out


class Rig:
    """Five RUNNING streams of kind ACC: a primer of 3 tokens of which 2 are still to be fed, two lead-sheet bars each, TARGET_BARS 2.  The two
    rows of a pair differ in their first primer token alone."""

    def __init__(self, V, seed, width=48, n_u=1024):
        self.V, self.width = V, width
        rs = np.random.RandomState(seed)
        self.pad, self.eos = PAD, EOS
        self.flags, self.beat = np.zeros(V, np.int32), np.zeros(V, np.int32)
        self.flags[BEAT0:BEAT0 + N_BEATS], self.beat[BEAT0:BEAT0 + N_BEATS] = 1, np.arange(N_BEATS)
        self.flags[TRACK_LS], self.flags[self.pad], self.flags[self.eos] = 2, 4, 8
        self.U = rs.rand(n_u, N).astype(np.float32)
        self.seq, self.segs = np.zeros((N, width), np.int64), np.zeros((N, width), np.int64)
        self.seq[:, :3] = [[0, 3, 4], [2, 3, 4], [1, 3, 4], [1, 7, 4], [2, 7, 4]]
        self.params, self.state = np.zeros((N, 8), np.int32), np.zeros((N, 8), np.int32)
        self.params[:, :5] = [[2, 1000, 0, 3 * r, 2] for r in range(N)]     # TARGET_BARS, MAX_EVENTS, SKIP_CHECK (off: Beats are checked), BAR0, N_BARS
        self.state[:, S_LEN], self.state[:, S_CONSUMED] = 3, 1
        toks, offs = [], []
        for r in range(N):
            for j in range(2):
                offs.append(len(toks))
                toks += [7, 26 if r < 3 else 27][:1 + j]                    # bar 1 (the injected one): two tokens, equal within a pair
            offs.append(len(toks))
        self.lead_tok, self.lead_off = np.array(toks, np.int64), np.array(offs, np.int32)

    def build(self, guide=False, scores=False, controls=None):
        from emo_disentanger_amd import ops
        t = self.t = dict(u_steps=T(self.U), ev_flags=T(self.flags), ev_beat=T(self.beat), params=T(self.params), state=T(self.state), seq=T(self.seq),
                          segs=T(self.segs), lead_tok=T(self.lead_tok), lead_off=T(self.lead_off),
                          tok_out=torch.full((N,), 1, dtype=torch.long, device=DEV), seg_out=torch.full((N,), -1, dtype=torch.long, device=DEV),
                          running=torch.tensor([N], dtype=torch.int32, device=DEV))
        self.logits = torch.zeros(N, self.V, device=DEV)
        num = dict(n_rows=N, n_token=self.V, ld_u=N, temperature=1.2, top_p=0.9, track_full=TRACK_FULL, max_len=self.width - 8, pad=self.pad)
        self.tabs = {}
        if scores:
            self.tabs = {k: torch.full((N, self.width), -1 if k == 'tok_rank' else float('nan'), device=DEV,
                                       dtype=torch.int32 if k == 'tok_rank' else torch.float32) for k in TABLES}
        more = {}
        if controls:
            num['n_masks'] = len(controls['tok_mask'])
            more = {k: T(v.view(np.int32) if k == 'tok_mask' else v) for k, v in controls.items()}
        if guide:
            more.update(guide_cond=T(COND), guide_uncond=T(UNCOND), guide_scale=T(SCALE))
        self.args, self.held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
        ops.block_set(self.args, self.held, logits=self.logits, **num, **t, **self.tabs, **more)
        return self

    def launch(self, logits):
        from emo_disentanger_amd import ops
        self.logits.copy_(T(np.ascontiguousarray(logits, dtype=np.float32)))
        ops.grammar_step(self.args)
        torch.cuda.synchronize()

    def snap(self):
        return {k: self.t[k].cpu().numpy().copy() for k in COMPARED}


def schedule(rig, rs, step):
    """The logits of launch `step`: two primer feeds, three Beat-heavy launches (a Beat that goes back is rejected and redrawn inside the launch),
    Track_LeadSheet (the next bar and Track_Full are injected and fed over the next launches), more draws, EOS at the last bar, one launch on
    finished streams."""
    heavy = step in (2, 3, 4)
    logits = (rs.randn(N, rig.V) * (0.5 if heavy else 2.0)).astype(np.float32)
    # (Beats: likely and alike in every row in three launches, so that none dominates a combined row and runs a stream into STUCK; absent elsewhere)
    logits[:, BEAT0:BEAT0 + N_BEATS] = (7.0 + 0.5 * rs.randn(N_BEATS)).astype(np.float32) if heavy else -BOOST
    logits[:, rig.pad] = 6.0 if heavy else -BOOST                              # PAD: a rejection that is not counted; alike in every row too
    logits[:, TRACK_LS] = BOOST if step == 7 else -BOOST                      # (never drawn by chance: every stream follows the schedule)
    logits[:, rig.eos] = BOOST if step == 13 else -BOOST
    return logits


def controls_for(V):
    """A ban row per pair (ids on both sides of a 32-bit word boundary, a Beat and the last id among them), per-stream temp / top_p, equal
    within a pair; stream 2 has no ban."""
    words = (V + 31) // 32
    mask = np.zeros((2, words), np.uint32)
    for m, ids in enumerate(([BEAT0, 31, 32, V - 1], [BEAT0 + 1, 0, 32])):
        for v in ids:
            mask[m, v >> 5] |= np.uint32(1 << (v & 31))
    return dict(tok_mask=mask, mask_of=np.array([0, 0, -1, 1, 1], np.int32), temp_of=np.array([0.9, 0.9, 1.2, 1.4, 1.4], np.float32),
                top_p_of=np.array([0.8, 0.8, 0.9, 0.95, 0.95], np.float32))


@pytest.mark.parametrize('ctl', [False, True], ids=['plain', 'controls'])
@pytest.mark.parametrize('V', [33, 327, 1024])
def test_a_guided_launch_is_the_unguided_launch_on_logits_combined_on_the_host(V, ctl):
    controls = controls_for(V) if ctl else None
    a = Rig(V, seed=V).build(guide=True, controls=controls)
    ref = Rig(V, seed=V)
    for r, (c, g, s) in PAIRS.items():
        ref.U[:, r] = ref.U[:, c]                                              # both rows of a pair read the leader's column
    ref.build(controls=controls)
    zero = Rig(V, seed=V)                                                      # scale 0: both rows hold the CONDITIONED logits, nothing is combined
    zero.U[:, 4] = zero.U[:, 3]
    zero.build(controls=controls)
    rs = np.random.RandomState(7 * V + ctl)
    redrew = fed = 0
    for step in range(15):
        logits = schedule(a, rs, step)
        s0 = a.t['state'].cpu().numpy().copy()
        a.launch(logits)
        comb = combined(logits)
        assert np.array_equal(comb[3].view(np.int32), logits[3].view(np.int32)) and np.array_equal(comb[4].view(np.int32), logits[3].view(np.int32))
        ref.launch(comb)
        plain = logits.copy()
        plain[4] = logits[3]
        zero.launch(plain)
        sa, sb, sz = a.snap(), ref.snap(), zero.snap()
        for k in COMPARED:
            assert np.array_equal(sa[k], sb[k]), (step, k, sa[k].tolist(), sb[k].tolist())
        # the pair invariant: the follower stays word for word with its leader, its first primer token apart
        for c, g in ((0, 1), (3, 4)):
            assert np.array_equal(sa['state'][c], sa['state'][g]) and np.array_equal(sa['seq'][c, 1:], sa['seq'][g, 1:]), (step, c, g)
            assert sa['tok_out'][c] == sa['tok_out'][g] and sa['seg_out'][c] == sa['seg_out'][g] and np.array_equal(sa['segs'][c], sa['segs'][g])
        assert sa['seq'][0, 0] == 0 and sa['seq'][1, 0] == 2
        for k in ('tok_out', 'seg_out'):
            assert np.array_equal(sa[k][3:], sz[k][3:]), (step, k)
        for k in ('state', 'seq', 'segs'):
            assert np.array_equal(sa[k][3:], sz[k][3:]), (step, k)
        s1 = sa['state']
        redrew += int(((s1[:, S_DRAWS] - s0[:, S_DRAWS]) > 1).sum())
        fed += int(((s1[:, S_CONSUMED] > s0[:, S_CONSUMED]) & (s1[:, S_DRAWS] == s0[:, S_DRAWS])).sum())
    st = a.t['state'].cpu().numpy()
    assert (st[:, S_STATUS] == 1).all() and int(a.t['running'].item()) == 0 and (st[:, S_BARS] == 1).all()      # the bar was injected, EOS closed every stream
    assert redrew >= 2 and fed >= 5 * N and (a.t['tok_out'].cpu().numpy() == a.pad).all()
    seq = a.t['seq'].cpu().numpy()
    assert (seq[np.arange(N), st[:, S_LEN] - 1] == a.eos).all()
    if ctl:
        drawn = seq[0, 3:st[0, S_LEN]].tolist()
        assert not set(drawn) & {BEAT0, 31, 32, V - 1}
    # the guidance moved a draw: the leader's ids are not those of its conditioned row alone
    alone = Rig(V, seed=V).build(controls=controls)
    rs = np.random.RandomState(7 * V + ctl)
    for step in range(15):
        alone.launch(schedule(alone, rs, step))
    assert not np.array_equal(alone.t['seq'].cpu().numpy()[0], seq[0])
    assert np.array_equal(alone.t['seq'].cpu().numpy()[2], seq[2]) and np.array_equal(alone.t['seq'].cpu().numpy()[3], seq[3])


def ref_scores(row, tok):
    l = row.astype(np.float64)
    mx = l.max()
    lse = mx + np.log(np.exp(l - mx).sum())
    p = np.exp(l - lse)
    return l[tok] - lse, int((l > l[tok]).sum() + (l[:tok] == l[tok]).sum()), lse - float((p * l).sum())


def test_the_scores_of_a_pair_are_each_rows_own_models_for_the_same_tokens():
    from emo_disentanger_amd import ops
    V = 327
    a = Rig(V, seed=11).build(guide=True, scores=True)
    rs = np.random.RandomState(12)
    hits = []
    for step in range(15):
        logits = schedule(a, rs, step)
        s0 = a.t['state'].cpu().numpy().copy()
        a.launch(logits)
        s1, seq = a.t['state'].cpu().numpy(), a.t['seq'].cpu().numpy()
        for r in range(N):
            if s1[r, S_ACCEPTED] > s0[r, S_ACCEPTED]:
                hits.append((r, int(s0[r, S_LEN]), int(seq[r, s0[r, S_LEN]]), logits[r].copy()))
    assert len(hits) >= 5 * N
    lp, rk, en = (a.tabs[k].cpu().numpy() for k in TABLES)
    cells = np.zeros((N, a.width), bool)
    for r, c, tok, row in hits:
        cells[r, c] = True
        logp, rank, ent = ref_scores(row, tok)                                  # the stream's OWN row, as the model wrote it
        assert rk[r, c] == rank, (r, c)
        assert abs(float(lp[r, c]) - logp) <= row_tol(row) and abs(float(en[r, c]) - ent) <= row_tol(row), (r, c)
    assert np.array_equal(rk >= 0, cells) and np.array_equal(~np.isnan(lp), cells) and np.array_equal(~np.isnan(en), cells)
    assert np.array_equal(cells[0], cells[1]) and np.array_equal(cells[3], cells[4]) and not cells[:, :3].any()
    ts = ops.token_scores(T(np.stack([h[3] for h in hits])), torch.tensor([h[2] for h in hits], device=DEV), -100, want=('rank', 'entropy'))
    nll, rank = ts['nll'].cpu().numpy(), ts['rank'].cpu().numpy()
    for i, (r, c, tok, row) in enumerate(hits):
        assert rk[r, c] == rank[i] and abs(float(lp[r, c]) + float(nll[i])) <= 2 * row_tol(row), (r, c)
    # the follower's figures are another model's for the same token: they differ from the leader's
    both = cells[0]
    assert not np.array_equal(lp[0][both], lp[1][both]) and not np.array_equal(rk[0][both], rk[1][both])


def test_with_the_three_fields_null_the_block_leaves_what_the_one_shot_step_leaves():
    from emo_disentanger_amd import ops
    V = 327
    a = Rig(V, seed=21).build(scores=True)
    b = Rig(V, seed=21).build(scores=True)
    assert a.args.guide_cond is None and a.args.guide_uncond is None and a.args.guide_scale is None
    rs = np.random.RandomState(22)
    for step in range(15):
        logits = schedule(a, rs, step)
        a.launch(logits)
        b.logits.copy_(T(logits))
        t = b.t                                                                 # a fresh block per call, built by the wrapper that never names the fields
        ops.acc_grammar_step(b.logits, 1.2, 0.9, t['u_steps'], t['ev_flags'], t['ev_beat'], t['lead_tok'], t['lead_off'], t['params'], t['state'],
                             t['seq'], t['segs'], b.width - 8, TRACK_FULL, b.pad, t['tok_out'], t['seg_out'], t['running'], **b.tabs)
        torch.cuda.synchronize()
        sa, sb = a.snap(), b.snap()
        for k in COMPARED:
            assert np.array_equal(sa[k], sb[k]), (step, k)
    for k in TABLES:
        assert np.array_equal(a.tabs[k].view(torch.int32).cpu().numpy(), b.tabs[k].view(torch.int32).cpu().numpy()), k
    assert int((a.tabs['tok_rank'] >= 0).sum().item()) >= 5 * N
