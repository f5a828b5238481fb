"""GPU: the optional sampling controls of emo_grammar_step (tok_mask / n_masks / mask_of / temp_of / top_p_of), kernel level, on synthetic fp32
logits and small synthetic event tables, all five kinds driven directly:
  - a masked launch on raw logits is bit for bit the unmasked launch on logits whose banned entries were overwritten with -inf, over several
    consecutive launches (primer feeds, in-launch redraws, endings, queue admissions);
  - each id drawn under a mask is the one tests/nucleus_ref.py (float64) gives on the masked row, under that file's tie and rounding rules;
  - per-stream temp_of / top_p_of equal one-row launches with those values as the block's scalars; the TXL key draw ignores them;
  - the recorded scores are the model's: taken from the RAW row.  emo_draw_scores.h states that its floats agree with emo_token_scores to
    rounding, not bit for bit (another reduction order), so "bit for bit" is held against what the launch without controls records for the
    same token of the same row, and emo_token_scores / float64 are held to the bounds tests/test_gpu_draw_scores.py holds them to;
  - with every new field NULL nothing changes."""
import numpy as np
import pytest
import torch

import nucleus_ref as nr

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TXL, ACC, WIN, TXLQ, ACCQ = 0, 1, 2, 3, 4
KINDS = [TXL, ACC, WIN, TXLQ, ACCQ]
S_LEN = 1
S_DRAWS = {TXL: 7, TXLQ: 7, ACC: 6, WIN: 6, ACCQ: 6}
S_ACCEPTED = {TXL: 2, TXLQ: 2, ACC: 7, WIN: 7, ACCQ: 7}
TABLES = ('tok_logp', 'tok_rank', 'tok_entropy')
ROW_TOL = 1e-5                       # tests/test_gpu_draw_scores.py: absolute, per row, at the logit scale randn x 3 (|l| < 16) ...
ULP16 = float(np.spacing(np.float32(15.99)))


def row_tol(row):
    """... scaled, as there, by the ulp of the row's largest |logit| where that is above the scale ROW_TOL was derived at."""
    return ROW_TOL * max(1.0, float(np.spacing(np.float32(np.abs(row).max()))) / ULP16)

COMPARED = ('tok_out', 'seg_out', 'state', 'seq', 'segs', 'running', 'slot_job', 'queue_head', 'mem_lens', 'row_reset', 'win_tok', 'win_seg')


def _ops():
    from emo_disentanger_amd import ops
    return ops


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def words(V):
    return (V + 31) // 32


def pack(ids, V, stray=False):
    """One row of tok_mask (emo_hip.h); stray: every bit at or beyond V in the last word set too."""
    row = np.zeros(words(V), np.uint32)
    for v in ids:
        row[v >> 5] |= np.uint32(1 << (v & 31))
    if stray and V % 32:
        row[-1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    return row


class Rig:
    """n streams (jobs, for the queue kinds: they run through `m` slots) of one kind.  Plain streams: RUNNING, a primer of L tokens of which the
    last is still to be fed (TXL, ACC: the launch after it draws).  Arrays may be changed (numpy) before build()."""

    def __init__(self, kind, V, n, m=None, L=2, width=40, n_u=96, seed=0):
        self.kind, self.V, self.n, self.L, self.width = kind, V, n, L, width
        self.queue = kind in (TXLQ, ACCQ)
        self.txl = kind in (TXL, TXLQ)
        self.m = n if m is None else m
        rs = np.random.RandomState(seed)
        self.flags, self.beat = np.zeros(V, np.int32), np.zeros(V, np.int32)
        self.pad = V - 2
        self.flags[self.pad] = 4                                   # EMO_TXL_EV_PAD == EMO_ACC_EV_PAD: a rejection (ACC kinds: a redraw in the launch)
        self.U = rs.rand(n_u, n).astype(np.float32)
        self.seq = np.zeros((n, width), np.int64)
        self.seq[:, :L] = rs.randint(0, V - 2, (n, L))
        self.segs = np.zeros((n, width), np.int64)
        self.params, self.state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
        if self.txl:
            self.params[:, :3] = 1000, 1000, L                     # MAX_BARS, MAX_EVENTS, PRIMER_LEN
            self.state[:, S_LEN], self.state[:, 6] = L, L - 1      # LEN, FEED
        else:
            self.params[:, :5] = 50, 1000, 0, 0, 1                 # TARGET_BARS, MAX_EVENTS, SKIP_CHECK, BAR0, N_BARS
            self.state[:, S_LEN], self.state[:, 2] = L, L - 1      # LEN, CONSUMED
        self.lead_tok, self.lead_off = np.zeros(4, np.int64), np.array([0, 2, 4], np.int32)
        self.rows = None
        self.temperature, self.top_p, self.key_temperature, self.key_top_p = 1.2, 0.9, 1.1, 0.97

    def one(self, r):
        """Stream r alone: a rig of one stream in one row with its tables, its column of the uniforms, its state."""
        o = Rig(self.kind, self.V, 1, 1, self.L, self.width)
        o.flags, o.beat, o.pad, o.lead_tok, o.lead_off = self.flags, self.beat, self.pad, self.lead_tok, self.lead_off
        o.U, o.seq, o.segs, o.params, o.state = self.U[:, r:r + 1], self.seq[r:r + 1], self.segs[r:r + 1], self.params[r:r + 1], self.state[r:r + 1]
        o.key_temperature, o.key_top_p = self.key_temperature, self.key_top_p
        return o

    def build(self, scores=False, raw_mask_of=None, **controls):
        """controls: tok_mask (uint32 numpy [n_masks, words]) / mask_of / temp_of / top_p_of, each optional.  raw_mask_of: a mask_of table written
        into the block behind block_set's back (it refuses rows outside the table; the kernel has to read them as -1)."""
        ops = _ops()
        n, m, V, kind = self.n, self.m, self.V, self.kind
        t = self.t = dict(u_steps=T(self.U), ev_flags=T(self.flags), ev_beat=T(self.beat), params=T(self.params), state=T(self.state),
                          seq=T(self.seq), running=torch.tensor([int((self.state[:, 0] == 0).sum())], dtype=torch.int32, device=DEV))
        self.logits = torch.zeros(m, V, device=DEV)
        num = dict(n_rows=m, n_token=V, ld_u=n, temperature=self.temperature, top_p=self.top_p)
        if self.txl:
            num.update(key_temperature=self.key_temperature, key_top_p=self.key_top_p)
            t.update(tok_out=torch.full((m,), 1, dtype=torch.long, device=DEV))
        else:
            num.update(track_full=0)
            t.update(segs=T(self.segs), lead_tok=T(self.lead_tok), lead_off=T(self.lead_off))
            if kind == WIN:
                num.update(window=2)
                t.update(win_tok=torch.full((m, 2), -1, dtype=torch.long, device=DEV), win_seg=torch.full((m, 2), -1, dtype=torch.long, device=DEV))
                if self.rows is not None:
                    t.update(rows=torch.tensor(self.rows, dtype=torch.int32, device=DEV))
            else:
                num.update(max_len=self.width - 8, pad=self.pad)
                t.update(tok_out=torch.full((m,), 1, dtype=torch.long, device=DEV), seg_out=torch.full((m,), -1, dtype=torch.long, device=DEV))
        if self.queue:
            num.update(n_jobs=n, mem_rows=64)
            t.update(slot_job=torch.full((m,), -1, dtype=torch.int32, device=DEV), queue_head=torch.zeros(1, dtype=torch.int32, device=DEV),
                     mem_lens=torch.zeros(m, dtype=torch.long, device=DEV))
            if kind == ACCQ:
                t.update(row_reset=torch.full((m,), 7, dtype=torch.int32, device=DEV))
        self.tabs = {}
        if scores:
            self.tabs = {k: torch.full((n, self.width), -1 if k == 'tok_rank' else float('nan'), device=DEV,
                                       dtype=torch.int32 if k == 'tok_rank' else torch.float32) for k in TABLES}
        ctl = {k: T(v.view(np.int32) if k == 'tok_mask' else v) for k, v in controls.items() if v is not None}
        if 'tok_mask' in ctl:
            num['n_masks'] = len(controls['tok_mask'])
        self.args, self.held = ops.GrammarStep(kind=kind), {}
        ops.block_set(self.args, self.held, logits=self.logits, **num, **t, **self.tabs, **ctl)
        if raw_mask_of is not None:
            self.held['mask_of'] = T(raw_mask_of)
            self.args.mask_of = self.held['mask_of'].data_ptr()
        return self

    def stream_of_row(self):
        """per row of the logits batch: the stream that draws from it in the next launch (-1: none)"""
        if self.queue:
            return [int(j) for j in self.t['slot_job'].cpu().tolist()]
        if self.kind == WIN and self.rows is not None:
            return list(self.rows)
        return list(range(self.m))

    def launch(self, logits):
        self.logits.copy_(T(np.ascontiguousarray(logits, dtype=np.float32)))
        _ops().grammar_step(self.args)
        torch.cuda.synchronize()

    def snap(self):
        """Every word the launch writes.  Queue kinds: which of several free slots gets which job is not specified (emo_hip.h), so the per-slot
        words are compared as the sorted (job, token, segment, position, reset flag) of the slots."""
        out = {k: v.cpu().numpy().copy() for k, v in self.t.items() if k in COMPARED}
        if self.queue:
            per_slot = [out.pop(k).tolist() for k in ('slot_job', 'tok_out', 'seg_out', 'mem_lens', 'row_reset') if k in out]
            out['slots'] = np.array(sorted(zip(*per_slot)))
        return out

    def batch(self, rs, scale=3.0):
        """Fresh logits for one launch.  Queue kinds: every slot sees the same row, so a job's ids do not depend on the slot it landed in."""
        if self.queue:
            return np.tile((rs.randn(self.V) * scale).astype(np.float32), (self.m, 1))
        return (rs.randn(self.m, self.V) * scale).astype(np.float32)


def masked(logits, rig, bans):
    """`logits` with the banned entries of the stream that draws from each row overwritten with -inf (bans: per stream, a list of ids or None)."""
    out = np.array(logits, dtype=np.float32)
    for b, r in enumerate(rig.stream_of_row()):
        if 0 <= r < rig.n and bans[r]:
            out[b, list(bans[r])] = -np.inf
    return out


# ------------------------------------------------------------------------------------------------ 1. mask equivalence
MASKS = ['none', 'argmax', 'last', 'all_but_one', 'all_but_two', 'stray']


def _case(mask, V, top, keep):
    """-> (the ids the case bans, stray bits)"""
    if mask == 'none':
        return [], False
    if mask == 'argmax':
        return [top], False
    if mask == 'last':
        return [V - 1], False
    if mask == 'all_but_one':
        return [v for v in range(V) if v != keep[0]], False
    if mask == 'all_but_two':
        return [v for v in range(V) if v not in keep], False
    return [top, 3, V - 1], True


@pytest.mark.parametrize('mask', MASKS)
@pytest.mark.parametrize('V', [33, 200, 327, 1024])
@pytest.mark.parametrize('kind', KINDS)
def test_a_masked_launch_is_the_unmasked_launch_on_minus_inf_logits(kind, V, mask):
    # streams 0 and 2 (and job 3 of a queue) draw under the case's mask, stream 1 under none; a second row of the table (another ban) is there and
    # unused by the case 'none', whose mask_of also holds values outside [-1, n_masks): read as -1.  Token `top` is the arg-max of every row, PAD
    # (a rejection: redrawn inside the launch by the ACC kinds) is likely, stream 0 ends early (MAX_EVENTS), so a queue admits its last job late.
    queue = kind in (TXLQ, ACCQ)
    n, m = (4, 3) if queue else (3, 3)
    top, keep = 7, (5, 11)
    ids, stray = _case(mask, V, top, keep)
    seed = 1000 * kind + V
    rigs = [Rig(kind, V, n, m, seed=seed) for _ in range(2)]
    for rig in rigs:
        rig.params[0, 1] = 4                                       # MAX_EVENTS: DONE once LEN > 4
        if kind == WIN:
            rig.rows = [2, 0, 1]
    table = np.stack([pack(ids, V, stray), pack([top + 1], V)])
    if mask == 'none':
        mask_of, bans = np.array([-1, 2, -9, 1000][:n], np.int32), [None] * n
    else:
        mask_of, bans = np.array([0, -1, 0, 0][:n], np.int32), [ids, None, ids, ids][:n]
    a = rigs[0].build(tok_mask=table, raw_mask_of=mask_of) if mask == 'none' else rigs[0].build(tok_mask=table, mask_of=mask_of)
    b = rigs[1].build()
    rs = np.random.RandomState(seed)
    redrew = ended = drew = 0
    for step in range(16):
        logits = a.batch(rs)
        logits[:, top] = logits.max(axis=1) + 1.0
        logits[:, a.pad] = logits[:, top] + (3.0 if step in (5, 6) else -2.0)      # (two launches in which PAD is the likeliest draw)
        s0 = a.t['state'].cpu().numpy().copy()
        a.launch(logits)
        b.launch(masked(logits, b, bans))
        sa, sb = a.snap(), b.snap()
        assert sa.keys() == sb.keys()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (step, k, sa[k].tolist(), sb[k].tolist())
        s1, seq = sa['state'], sa['seq']
        d = s1[:, S_DRAWS[kind]] - s0[:, S_DRAWS[kind]]
        redrew += int((d > 1).sum())
        ended += int(((s1[:, 0] != 0) & (s0[:, 0] == 0)).sum())
        for r in range(n):
            if s1[r, S_ACCEPTED[kind]] > s0[r, S_ACCEPTED[kind]]:
                drew += 1
                tok = int(seq[r, s0[r, S_LEN]])
                if bans[r]:
                    assert tok not in bans[r], (step, r, tok)
                    if mask == 'all_but_one':
                        assert tok == keep[0]                      # whatever u is
                    if mask == 'all_but_two':
                        assert tok in keep
    assert drew >= 8 and ended >= 1
    if kind in (ACC, WIN, ACCQ) and mask in ('none', 'argmax', 'last', 'stray'):
        assert redrew >= 1                                         # a launch that drew PAD and drew again from the masked sort
    if queue:
        assert int(a.t['queue_head'].item()) >= n                  # the last job was admitted on the way


# ------------------------------------------------------------------------------------------------ 2. float64 reference
@pytest.mark.parametrize('V, scale, temp, top_p', [(33, 2.0, 1.2, 0.9), (200, 2.0, 1.2, 0.9), (327, 4.0, 1.1, 0.9), (1024, 4.0, 1.0, 0.97)])
@pytest.mark.parametrize('kind', [TXL, ACC])
def test_ids_drawn_under_a_mask_are_the_float64_samplers_on_the_masked_row(kind, V, scale, temp, top_p):
    # one row of logits, a third of it banned (the arg-max and the last id among them); every probe of nucleus_ref.Row on the MASKED row is a
    # stream of one launch on the RAW row.  No event is special: every draw is accepted.
    rng = np.random.default_rng(V + kind)
    for trial in range(3):
        raw = nr.family_rows(rng, V, scale, 1)[0]
        ban = sorted(set(rng.choice(V, size=V // 3, replace=False).tolist()) | {int(raw.argmax()), V - 1})
        row = raw.copy()
        row[ban] = -np.inf
        ref = nr.Row(row, temp, top_p)
        u, _ = ref.probes()
        R = len(u)
        rig = Rig(kind, V, R, L=2, width=16, n_u=1)
        rig.flags[:] = 0
        rig.U = u.reshape(1, R).copy()
        rig.state[:, 6 if kind == TXL else 2] = 2                  # the primer is fed: this launch draws
        rig.temperature, rig.top_p = temp, top_p
        rig.build(tok_mask=np.stack([pack(ban, V, True)]), mask_of=np.zeros(R, np.int32))
        rig.launch(np.tile(raw, (R, 1)))
        st, seq = rig.t['state'].cpu().numpy(), rig.t['seq'].cpu().numpy()
        assert (st[:, S_LEN] == 3).all()
        got = seq[:, 2]
        assert not set(got.tolist()) & set(ban)
        ref.check(u, got)


# ------------------------------------------------------------------------------------------------ 3. per-stream parameters
def _drive(rig, rows_logits, steps, rs_seed):
    rs = np.random.RandomState(rs_seed)
    out = []
    for step in range(steps):
        row = (rs.randn(rig.V) * 3).astype(np.float32)             # every row of the batch sees the same logits: a job's ids do not depend on its slot
        rig.launch(np.tile(row, (rows_logits, 1)))
        out.append({k: rig.t[k].cpu().numpy().copy() for k in ('state', 'seq')})
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_per_stream_temperature_and_top_p_equal_one_row_launches_with_the_scalars(kind):
    V, n = 200, 3
    temps, top_ps = np.array([0.7, 1.2, 2.5], np.float32), np.array([0.5, 0.9, 1.0], np.float32)
    full = Rig(kind, V, n, seed=50 + kind)
    full.temperature, full.top_p = 9.0, 0.123                      # the block's scalars are replaced for every stream
    full.build(temp_of=temps, top_p_of=top_ps)
    got = _drive(full, n, 8, 77)
    differ = 0
    for r in range(n):
        one = Rig(kind, V, n, seed=50 + kind).one(r)
        one.temperature, one.top_p = float(temps[r]), float(top_ps[r])
        one.build()
        for step, (g, w) in enumerate(zip(got, _drive(one, 1, 8, 77))):
            assert np.array_equal(g['state'][r], w['state'][0]), (r, step, g['state'][r].tolist(), w['state'][0].tolist())
            assert np.array_equal(g['seq'][r], w['seq'][0]), (r, step)
        # ... and not those of another stream's values (same uniforms, same logits)
        other = Rig(kind, V, n, seed=50 + kind).one(r)
        other.temperature, other.top_p = float(temps[(r + 1) % n]), float(top_ps[(r + 1) % n])
        other.build()
        differ += int(not np.array_equal(_drive(other, 1, 8, 77)[-1]['seq'][0], got[-1]['seq'][r]))
    assert differ >= 2
    # one of the two alone leaves the other to the block's scalar
    half = Rig(kind, V, n, seed=50 + kind)
    half.temperature, half.top_p = 9.0, float(top_ps[1])
    half.build(temp_of=temps)
    h = _drive(half, n, 8, 77)
    assert np.array_equal(h[-1]['seq'][1], got[-1]['seq'][1]) and np.array_equal(h[-1]['state'][1], got[-1]['state'][1])


def test_the_txl_key_draw_keeps_the_key_temperature_and_obeys_the_ban():
    V, n = 200, 3
    key = 20

    def rig(temperature, top_p, **ctl):
        g = Rig(TXL, V, n, L=1, seed=9)
        g.flags[:] = 0
        g.params[:, 3] = 1                                         # KEYED: with LEN == 1 the next draw is the key draw
        g.state[:, 6] = 1                                          # the one primer token is fed
        g.temperature, g.top_p, g.key_temperature, g.key_top_p = temperature, top_p, 1.1, 0.97
        return g.build(**ctl)

    rs = np.random.RandomState(4)
    logits = (rs.randn(n, V) * 2).astype(np.float32)
    a = rig(1.2, 0.9)
    b = rig(7.0, 0.2, temp_of=np.array([0.3, 5.0, 9.0], np.float32), top_p_of=np.array([0.1, 0.2, 0.3], np.float32))
    a.launch(logits)
    b.launch(logits)
    sa, sb = a.snap(), b.snap()
    assert (sa['state'][:, S_LEN] == 2).all()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k                     # the key draw: key_temperature / key_top_p, whatever temp_of / top_p_of hold
    logits2 = (rs.randn(n, V) * 2).astype(np.float32)
    a.launch(logits2)
    b.launch(logits2)
    assert not np.array_equal(a.snap()['seq'], b.snap()['seq'])    # the draw after it: the streams' own values
    # the ban holds for the key draw: every token but `key` banned -> the key is drawn
    c = rig(1.2, 0.9, tok_mask=np.stack([pack([v for v in range(V) if v != key], V)]), mask_of=np.array([0, -1, 0], np.int32))
    c.launch(logits)
    sc = c.snap()
    assert sc['seq'][[0, 2], 1].tolist() == [key, key] and sc['seq'][1, 1] == sa['seq'][1, 1]


# ------------------------------------------------------------------------------------------------ 4. scores
def ref_scores(row, tok):
    l = row.astype(np.float64)
    mx = l.max()
    lse = mx + np.log(np.exp(l - mx).sum())
    p = np.exp(l - lse)
    return l[tok] - lse, int((l > l[tok]).sum() + (l[:tok] == l[tok]).sum()), lse - float((p * l).sum())


def _bits(t):
    return t.view(torch.int32).cpu().numpy().copy()


@pytest.mark.parametrize('kind', KINDS)
def test_the_scores_under_a_mask_are_the_models_from_the_raw_row(kind):
    ops = _ops()
    V = 327
    queue = kind in (TXLQ, ACCQ)
    n, m = (4, 3) if queue else (3, 3)
    top = 7
    low = [100, 101, 102]                                          # at -60: exp() of them is below half an ulp of every partial sum, so
                                                                   # banning them changes no bit of the draw's arithmetic
    hard = Rig(kind, V, n, m, seed=3).build(scores=True, tok_mask=np.stack([pack([top], V)]), mask_of=np.zeros(n, np.int32))
    soft = Rig(kind, V, n, m, seed=3).build(scores=True, tok_mask=np.stack([pack(low, V, True)]), mask_of=np.zeros(n, np.int32))
    plain = Rig(kind, V, n, m, seed=3).build(scores=True)
    rs = np.random.RandomState(8)
    hits = []
    for step in range(8):
        logits = hard.batch(rs)
        logits[:, top] = logits.max(axis=1) + 1.0
        logits[:, low] = -60.0
        s0 = hard.t['state'].cpu().numpy().copy()
        of_row = hard.stream_of_row()
        for g in (hard, soft, plain):
            g.launch(logits)
        s1, seq = hard.t['state'].cpu().numpy(), hard.t['seq'].cpu().numpy()
        for r in range(n):
            if s1[r, S_ACCEPTED[kind]] > s0[r, S_ACCEPTED[kind]]:
                c = int(s0[r, S_LEN])
                hits.append((r, c, int(seq[r, c]), logits[of_row.index(r)]))
    # (a) bans that move no draw: ids, state and the three tables are bit for bit those of the launch without controls
    for k in ('state', 'seq'):
        assert np.array_equal(soft.t[k].cpu().numpy(), plain.t[k].cpu().numpy()), k
    for k in TABLES:
        assert np.array_equal(_bits(soft.tabs[k]), _bits(plain.tabs[k])), k
    assert int((plain.tabs['tok_rank'] >= 0).sum().item()) >= 8
    # (b) the arg-max banned: exactly the accepted cells are written, with the figures of the RAW row (the banned arg-max still counts in the
    # rank and in the normaliser); cells of given tokens keep the caller's fill
    assert len(hits) >= 8
    lp, rk, en = (hard.tabs[k].cpu().numpy() for k in TABLES)
    cells = np.zeros((n, hard.width), bool)
    for r, c, tok, row in hits:
        assert tok != top
        cells[r, c] = True
        logp, rank, ent = ref_scores(row, tok)
        assert rk[r, c] == rank and rank >= 1
        assert abs(float(lp[r, c]) - logp) <= row_tol(row) and abs(float(en[r, c]) - ent) <= row_tol(row)
    assert np.array_equal(rk >= 0, cells) and np.array_equal(~np.isnan(lp), cells) and np.array_equal(~np.isnan(en), cells)
    assert not cells[:, :2].any()                                  # the primer
    ts = ops.token_scores(T(np.stack([h[3] for h in hits])), torch.tensor([h[2] for h in hits], device=DEV), -100, want=('rank', 'entropy'))
    nll, rank = ts['nll'].cpu().numpy(), ts['rank'].cpu().numpy()
    for i, (r, c, tok, row) in enumerate(hits):
        assert rk[r, c] == rank[i] and abs(float(lp[r, c]) + float(nll[i])) <= 2 * row_tol(row)


# ------------------------------------------------------------------------------------------------ 5. all fields NULL
@pytest.mark.parametrize('kind', KINDS)
def test_with_every_new_field_null_the_block_is_the_one_without_them(kind):
    from emo_disentanger_amd import _lib
    queue = kind in (TXLQ, ACCQ)
    n, m = (4, 3) if queue else (3, 3)
    a = Rig(kind, 200, n, m, seed=5).build(scores=True)
    b = Rig(kind, 200, n, m, seed=5).build(scores=True, tok_mask=None, mask_of=None, temp_of=None, top_p_of=None)
    # a block that never heard of the fields: the bytes a zero-initialised struct has there
    for k in ('tok_mask', 'mask_of', 'temp_of', 'top_p_of'):
        assert getattr(a.args, k) is None and getattr(b.args, k) is None
    assert a.args.n_masks == 0 and isinstance(a.args, _lib.GrammarStep)
    b.args.n_masks = 5                                             # without tok_mask the count is not read
    rs = np.random.RandomState(6)
    for step in range(8):
        logits = a.batch(rs)
        a.launch(logits)
        b.launch(logits)
        sa, sb = a.snap(), b.snap()
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (step, k)
    for k in TABLES:
        assert np.array_equal(_bits(a.tabs[k]), _bits(b.tabs[k]))
    assert int((a.tabs['tok_rank'] >= 0).sum().item()) >= 8
