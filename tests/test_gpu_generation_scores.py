"""GPU: the scores the grammar launch records at each draw, through the generators — generate_lead_sheets / generate_accompaniments
(return_scores=True) return the ids of the calls without it; the recorded log-probabilities against the scoring forwards over the finished
pieces (scoring.score_lead_sheet_tokens, scoring.score_tokens), past the window against the window forward's own logits; best_by='draws'.
Tiny models and vocabularies of the existing generation tests."""
import numpy as np
import pytest
import torch

from test_gpu_stage1_scoring import _generator_fixture
from test_gpu_stage2_window import _tiny, _tiny_batch, _vocab

pytestmark = pytest.mark.gpu

# Measured on MI355X (the figure each test prints), asserted at 2 x the measurement, the project's convention for measured bounds: the largest
# |recorded logp - scoring forward's logp| over all drawn tokens of the test's pieces.  Both sides are fp32 model passes over the same tokens
# in different forms (one-token steps on a cache / one banded or causal forward), so they differ by the rounding of the logits, not by more.
# stage 1, per (step, reference): 'steps' = float64 on the logits of a second run of one-token decode_step calls fed exactly what the loop fed
# (re-fed tokens after a rejection included), every drawn token; 'forward' = score_lead_sheet_tokens, the drawn tokens in front of each stream's
# first rejection.  chain: the tiny fp32 generator (261 draws, 116 of them behind a rejection; 130 in front of a first one; all ranks equal).
# one_launch: d 512 / 2 layers / bf16, the shape emo_decode_step[txl] takes: its restatement runs the same one-launch step on a memory of its
# own, so its rows are the rows the draws were made from and the bound is the launch's own on a given row (row_tol of
# tests/test_gpu_draw_scores.py); the banded forward is the fp32 check and is not repeated in bf16.
STAGE1_MEASURED = {('chain', 'steps'): 5.242e-7, ('chain', 'forward'): 9.537e-7}
STAGE2_MEASURED = 2.861e-6   # 818 drawn tokens of 6 pieces; ranks equal at all 818
# Past the window the reference is float64 on the logits of a one-row window forward: the recorded figure is within ROW_TOL of float64 on the
# row it was drawn from (tests/test_gpu_draw_scores.py, the bound of emo_token_scores at this logit scale), and the batched forward's row
# differs from the one-row forward's only by the rounding of its GEMMs (measured: 3.2e-7 in total).
ROW_TOL = 1e-5

S1_PRIMERS = [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Positive'], ['Emotion_Negative', 'Key_a'], ['Emotion_Negative'], ['Emotion_Q1']]
S1_KW = dict(max_bars=4, max_events=60, temp=1.2, top_p=0.9, representation='functional', seed=11)


def ok(r):
    return isinstance(r, list)


def same(a, b):
    return a == b if ok(a) or ok(b) else type(a) is type(b)


def drawn(sc):
    return (sc['rank'] >= 0) & ~np.isnan(sc['logp'])


def margin(l64, tok):
    """Distance from the accepted logit to its nearest neighbour in the reference row (float64 numpy)."""
    d = np.abs(l64 - l64[tok])
    d[tok] = np.inf
    return float(d.min())


def log_softmax64(row):
    l = row.double().cpu().numpy()
    mx = l.max()
    return l - (mx + np.log(np.exp(l - mx).sum())), l


class Ranks:
    """The rank rule: equal wherever the reference's margin between the accepted logit and its neighbours exceeds the logp bound; the share of
    positions so compared is reported and must be at least one half."""

    def __init__(self):
        self.n = self.compared = 0

    def add(self, got, ref, mg, logp_bound):
        self.n += 1
        if mg > logp_bound:
            self.compared += 1
            assert int(got) == int(ref), 'rank %d against the reference\'s %d at a margin of %.3e (bound %.3e)' % (got, ref, mg, logp_bound)

    def check(self, what):
        print('[measured] %s: ranks compared (and equal) at %d of %d positions' % (what, self.compared, self.n))
        assert 2 * self.compared >= self.n


def bound(measured, err, what):
    print('[measured] %s: max |recorded - forward| = %.3e' % (what, err))
    assert measured is not None, 'no measured bound recorded for %s (this run: %.3e)' % (what, err)
    assert err <= 2 * measured, '%s: %.3e above 2 x the measured %.3e' % (what, err, measured)


# ------------------------------------------------------------------------------------------------ 1. ids unchanged
def test_return_scores_leaves_the_ids_as_they_are():
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    m, e2i, i2e = _generator_fixture()
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, S1_PRIMERS, **S1_KW)
    got, _, sc = s1.generate_lead_sheets(m, e2i, i2e, S1_PRIMERS, return_scores=True, **S1_KW)
    assert all(same(a, b) for a, b in zip(plain, got)) and sum(ok(r) for r in got) >= 3
    for ids, s, p in zip(got, sc, S1_PRIMERS):
        assert (s is None) == (not ok(ids))
        if ok(ids):
            assert all(len(s[k]) == len(ids) for k in ('logp', 'rank', 'entropy'))
            d = drawn(s)
            assert not d[:len(p)].any() and d[len(p):].all()                   # the primer was given, everything behind it drawn
            assert (s['logp'][d] <= 0).all() and (s['entropy'][d] >= 0).all() and np.isnan(s['entropy'][~d]).all()
    g, e2i, i2e = _vocab()
    model = _tiny('gpt2', 'fp32')
    leads, primers = _tiny_batch(g)
    kw = dict(max_events=150, skip_check=False, temp=1.2, top_p=0.97, seed=5)
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **kw)
    got, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, return_scores=True, **kw)
    assert got == plain and all(ok(r) for r in got)
    tf, tls = e2i['Track_Full'], e2i['Track_LeadSheet']
    for ids, s in zip(got, sc):
        d = drawn(s)
        assert len(d) == len(ids) and d.any()
        # a drawn token lies inside a Track_Full span (Track_LeadSheet, which closes it, included); the Track_Full that opens a span was injected
        # (one drawn inside a span is an ordinary event)
        inside = False
        for t, was_drawn in zip(ids, d):
            assert was_drawn == inside, (t, was_drawn, inside)
            inside = True if t == tf else False if t == tls else inside


# ------------------------------------------------------------------------------------------------ 2. stage 1
def _stage1_case(step):
    from emo_disentanger_amd import stage1_inference as s1
    if step == 'chain':
        m, e2i, i2e = _generator_fixture()
        primers = [p for p in S1_PRIMERS if len(p) == 1] * 3
        return m, e2i, i2e, primers, S1_KW
    from test_gpu_stage1_batch import _synthetic_vocab
    from test_gpu_stage1_one_launch import _model, _sd
    m = _model(2, 64, sd=_sd(2))
    e2i, i2e = _synthetic_vocab()
    primers = [['Emotion_%s' % e] for e in ('Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative')] * 2
    why = s1.one_launch_unsupported(m, len(primers))
    if why is not None:
        pytest.skip("step='one_launch' needs %s" % why)
    return m, e2i, i2e, primers, dict(max_bars=4, max_events=60, temp=1.2, top_p=0.9, representation='functional', seed=11)


@pytest.mark.parametrize('step', ['chain', 'one_launch'])
def test_stage1_recorded_scores_are_what_the_generating_steps_assigned(step):
    # The loop is stepped by hand.  Beside it runs the restatement: a second memory, prefilled alike, and one token step of the same form
    # (decode_step, or a second OneLaunchStep) on exactly the token the loop fed — after a rejection the previous input again, as the reference's loop
    # does.  Its logits in float64 are the reference for EVERY drawn token, the ones behind a rejection included.  score_lead_sheet_tokens on
    # the finished pieces is the second reference, up to each stream's first rejected draw: from there on the memory holds a token the piece
    # does not, and a forward over the piece ("no rejected draws") is a different computation.
    from emo_disentanger_amd import scoring, stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import TXLMemory
    from test_gpu_draw_scores import row_tol
    m, e2i, i2e, primers, kw = _stage1_case(step)
    loop = s1.LeadSheetLoop(m, e2i, i2e, primers, step=step, scores=True, **kw)
    n, L0 = loop.n, loop.L0
    first = [None] * n                                                        # the length a stream had at its first rejected draw
    b_steps = STAGE1_MEASURED.get((step, 'steps'))
    b_fwd = STAGE1_MEASURED.get((step, 'forward'))
    ranks, err, hits, margins = Ranks(), 0.0, 0, {}
    with torch.no_grad():
        mem2 = TXLMemory(m, n, m._max_gen_len)
        h, _, _ = m._prefill(loop.seq[:, :L0].t(), mem2)
        ref = m._logits(h.view(n, L0, -1)[:, -1].contiguous()).float().clone()
        step2 = s1.OneLaunchStep(m, n, loop.max_len, r_dist=mem2.r_dist).take_over(mem2, L0) if step == 'one_launch' else None
        while loop._live() > 0:
            before = loop.state.cpu().numpy().copy()
            loop.grammar()
            after, seq = loop.state.cpu().numpy(), loop.seq.cpu().numpy()
            for i in range(n):
                if after[i, s1.S_DRAWS] == before[i, s1.S_DRAWS]:
                    continue
                if after[i, s1.S_ACCEPTED] == before[i, s1.S_ACCEPTED]:
                    if first[i] is None:
                        first[i] = int(before[i, s1.S_LEN])
                    continue
                c = int(before[i, s1.S_LEN])
                tok = int(seq[i, c])
                lsm, l64 = log_softmax64(ref[i])
                tol = row_tol(l64)
                e = abs(float(loop.score_tables['tok_logp'][i, c].item()) - lsm[tok])
                assert step == 'chain' or e <= tol, (i, c, e, tol)
                err = max(err, e)
                margins[(i, c)] = margin(l64, tok)
                ranks.add(loop.score_tables['tok_rank'][i, c].item(), (l64 > l64[tok]).sum() + (l64[:tok] == l64[tok]).sum(), margins[(i, c)],
                          2 * b_steps if step == 'chain' else tol)
                hits += 1
            if loop._live() == 0 or loop.pos >= loop.max_len:
                break
            tok_in = loop.tok.clone()
            if loop.stepper is not None:
                loop.stepper.step(loop.tok, logits_out=loop.logits)
            else:
                m.decode_step(loop.tok, loop.mem, logits_out=loop.logits)
            ref = (m.decode_step(tok_in, mem2) if step2 is None else step2.step(tok_in)).float().clone()
            loop.pos += 1
    if loop.stepper is not None:
        loop.stepper.check_persistent()
        step2.check_persistent()
    got, sc = loop.results(), loop.scores()
    keep = [i for i, r in enumerate(got) if ok(r)]
    behind = sum(int((np.flatnonzero(drawn(sc[i])) >= first[i]).sum()) for i in keep if first[i] is not None)
    print('[measured] stage 1 [%s]: %d accepted draws held to the stepped reference, %d of them (finished pieces) behind a rejection' % (step, hits, behind))
    assert (len(keep) >= 4 and hits >= 60 and behind >= 20) if step == 'chain' else (len(keep) >= 1 and hits >= 30 and behind >= 1)
    assert hits >= sum(int(drawn(sc[i]).sum()) for i in keep)                 # every drawn token of every result was one of them
    ranks.check('stage 1 [%s] against the stepped float64 reference' % step)
    print('[measured] stage 1 [%s]: stepped reference max |recorded - float64| = %.3e' % (step, err))
    if step != 'chain':
        return
    # the banded forward over the finished pieces, in front of the first rejection
    pad = m.n_token - 1
    T = max(len(got[i]) for i in keep)
    tok = np.full((len(keep), T), pad, np.int64)
    for b, i in enumerate(keep):
        tok[b, :len(got[i])] = got[i]
    fw = scoring.score_lead_sheet_tokens(m, torch.from_numpy(tok).cuda(), [len(got[i]) for i in keep], [len(primers[i]) for i in keep])
    lp, rk, mask = fw.logprob.cpu().numpy(), fw.rank.cpu().numpy(), fw.mask.cpu().numpy()
    err_f, err_b, n_f, ranks_f = 0.0, 0.0, 0, Ranks()
    for b, i in enumerate(keep):
        d = drawn(sc[i])
        assert int(mask[b].sum()) == int(d.sum())                             # the forward's targets ARE the drawn tokens
        for c in np.flatnonzero(d):                                           # entry (b, c - 1) of the forward scores token c
            e = abs(float(sc[i]['logp'][c]) - float(lp[b, c - 1]))
            if first[i] is not None and c >= first[i]:
                err_b = max(err_b, e)
                continue
            err_f = max(err_f, e)
            n_f += 1
            ranks_f.add(sc[i]['rank'][c], rk[b, c - 1], margins[(i, int(c))], 2 * (b_fwd or 0.0))
    print('[measured] stage 1 [%s]: banded forward, %d tokens in front of a first rejection; behind one the two differ by up to %.3e' % (step, n_f, err_b))
    assert n_f >= 20
    ranks_f.check('stage 1 [%s] against score_lead_sheet_tokens' % step)
    print('[measured] stage 1 [%s]: forward max |recorded - forward| = %.3e' % (step, err_f))
    bound(b_steps, err, 'stage 1, %s step, stepped float64 reference' % step)
    bound(b_fwd, err_f, 'stage 1, %s step, banded forward' % step)


# ------------------------------------------------------------------------------------------------ 3. stage 2, GPT-2 fp32
def test_stage2_recorded_logp_is_what_the_scoring_forward_assigns():
    from emo_disentanger_amd import inference as inf, scoring
    g, e2i, i2e = _vocab()
    model = _tiny('gpt2', 'fp32')
    leads, primers = _tiny_batch(g)
    kw = dict(max_events=150, skip_check=False, temp=1.2, top_p=0.97, seed=5)
    got, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, return_scores=True, **kw)
    pad = model.n_token - 1
    err, n, ranks = 0.0, 0, Ranks()
    for ids, s in zip(got, sc):
        inp, tgt, seg = scoring.targets_of(ids, e2i, inf.max_dec_inp_len, pad)
        fw = scoring.score_tokens(model, torch.from_numpy(inp)[None].cuda(), torch.from_numpy(tgt)[None].cuda(),
                                  seg_inp=torch.from_numpy(seg)[None].cuda(), pad_token=pad)
        lp, rk = fw.logprob[0].cpu().numpy(), fw.rank[0].cpu().numpy()
        with torch.no_grad():                                                 # the same forward again, for the margins of its rows
            lg = model(torch.from_numpy(inp)[None].cuda(), seg_inp=torch.from_numpy(seg)[None].cuda())[0].double().cpu().numpy()
        for c in np.flatnonzero(drawn(s)):
            if c >= len(inp):
                continue
            assert tgt[c - 1] == ids[c]                                       # the forward's target at c - 1 is the drawn token at c
            err = max(err, abs(float(s['logp'][c]) - float(lp[c - 1])))
            ranks.add(s['rank'][c], rk[c - 1], margin(lg[c - 1], ids[c]), 2 * STAGE2_MEASURED)
            n += 1
    assert n >= 100
    ranks.check('stage 2, GPT-2 fp32, against score_tokens')
    bound(STAGE2_MEASURED, err, 'stage 2, GPT-2 fp32')


# ------------------------------------------------------------------------------------------------ 4. stage 2, Performer with redraw
def test_performer_with_redraw_records_the_probabilities_under_the_engine_s_own_feature_map():
    # A Performer that redraws its random features on every forward: the engine draws one map for the piece and keeps it, a scoring forward
    # afterwards draws another.  The loop is stepped by hand; beside it runs the restatement, a second engine (the chain of launches) holding
    # the SAME feature maps and fed exactly what the loop fed.  The recorded figures equal float64 on its logits, within the bound
    # tests/test_gpu_draw_scores.py holds the launch to on a given row (row_tol), with exact ranks.  Two score_tokens calls on the finished
    # pieces differ from each other by far more: the gap the recorded scores close.
    from test_gpu_draw_scores import ref_scores, row_tol
    from emo_disentanger_amd import inference as inf, scoring
    g, e2i, i2e = _vocab()
    model = _tiny('performer', 'fp32')
    model.redraw = 'every_forward'
    lead = [list(b) for b in g['lead']]
    leads, primers = [lead, lead[::-1], lead[:2]], [list(g['primer']), [1, 5, 6], [2, 4, 6]]
    kw = dict(max_events=150, skip_check=False, temp=1.2, top_p=0.97, seed=5)
    before_maps = [lyr.attention.inner_attention.feature_map.omega.clone() for lyr in model.transformer_decoder.decoder_layers]
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, scores=True, **kw)
    maps = [o.clone() for o in loop.eng.omegas]
    assert not any(torch.equal(a, b) for a, b in zip(before_maps, maps))      # the engine drew its own
    n, L0 = loop.n, loop.L0
    err, hits = 0.0, 0
    with torch.no_grad():
        eng2 = inf.PerformerDecodeEngine(model, n, redraw=False, persistent=False)
        eng2.omegas = [o.clone() for o in maps]
        eng2.max_len = loop.W
        ref = eng2.prefill(loop.seq[:, :L0].contiguous(), loop.segs[:, :L0].contiguous()).float().clone()
        while loop._live() > 0:
            before = loop.state.cpu().numpy().copy()
            loop.grammar()
            after, seq = loop.state.cpu().numpy(), loop.seq.cpu().numpy()
            rows = ref.cpu().numpy()
            for i in range(n):
                if after[i, inf.ACC_S_ACCEPTED] == before[i, inf.ACC_S_ACCEPTED]:
                    continue
                c = int(before[i, inf.ACC_S_LEN])
                tok = int(seq[i, c])
                logp, rank, ent = ref_scores(rows[i], tok)
                tol = row_tol(rows[i])
                e = max(abs(float(loop.score_tables['tok_logp'][i, c].item()) - logp), abs(float(loop.score_tables['tok_entropy'][i, c].item()) - ent))
                assert e <= tol, (i, c, e, tol)
                assert loop.score_tables['tok_rank'][i, c].item() == rank
                err = max(err, e)
                hits += 1
            if loop._live() == 0 or loop.pos >= loop.bound:
                break
            tok_in, seg_in = loop.tok.clone(), loop.segv.clone()
            loop.eng.step(loop.tok, loop.segv, dev_pos=True, logits_out=loop.logits)
            ref = eng2.step(tok_in, seg_in).float().clone()
            loop.pos += 1
    assert all(torch.equal(a, b) for a, b in zip(maps, loop.eng.omegas))
    out = loop.results(e2i, i2e, 150, False, 5)
    sc = loop.scores(out)
    assert all(ok(r) for r in out) and hits >= 40
    pad = model.n_token - 1
    spread = dev = 0.0
    for ids, s in zip(out, sc):
        inp, tgt, seg = (torch.from_numpy(a)[None].cuda() for a in scoring.targets_of(ids, e2i, inf.max_dec_inp_len, pad))
        a = scoring.score_tokens(model, inp, tgt, seg_inp=seg, pad_token=pad).logprob[0].cpu().numpy()
        b = scoring.score_tokens(model, inp, tgt, seg_inp=seg, pad_token=pad).logprob[0].cpu().numpy()
        cols = np.flatnonzero(drawn(s))
        spread = max(spread, float(np.abs(a[cols - 1] - b[cols - 1]).max()))
        dev = max(dev, float(np.abs(s['logp'][cols] - a[cols - 1]).max()))
    print('[measured] Performer with redraw: %d draws, max |recorded - float64 on the engine\'s logits| = %.3e; two score_tokens calls differ by %.3e, '
          'recorded and one of them by %.3e' % (hits, err, spread, dev))
    assert spread > err


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_full_shape_one_launch_engines_record_scores_and_keep_their_ids(kind):
    # the benchmark shape, where the engine step is the one persistent launch and the loop replays hipGraphs: the tables ride along
    from test_gpu_stage2_batch import _full_batch, _full_model, _full_vocab
    from emo_disentanger_amd import inference as inf
    e2i, i2e = _full_vocab()
    model = _full_model(kind)
    leads, primers = _full_batch(e2i, n=8)
    kw = dict(max_events=10000, skip_check=False, temp=1.2, top_p=0.9, seed=11)
    plain = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, scores=True, **kw)
    assert loop.eng.persist is not None
    plain.run(use_graph=True)
    loop.run(use_graph=True)
    out = loop.results(e2i, i2e, 10000, False, 11)
    assert out == plain.results(e2i, i2e, 10000, False, 11) and sum(ok(r) for r in out) >= 6
    st = loop.state.cpu().numpy()
    rank = loop.score_tables['tok_rank'].cpu().numpy()
    assert ((rank >= 0).sum(1) == st[:, inf.ACC_S_ACCEPTED]).all() and (st[:, inf.ACC_S_ACCEPTED] > 0).all()
    for ids, s in zip(out, loop.scores(out)):
        if ok(ids):
            d = drawn(s)
            assert d.any() and np.isfinite(s['logp'][d]).all() and (s['logp'][d] <= 0).all() and (s['entropy'][d] >= 0).all()


# ------------------------------------------------------------------------------------------------ 5. past the window
def test_scores_cross_the_window_with_their_tokens(monkeypatch):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    model = _tiny('gpt2', 'fp32')
    leads, primers = _tiny_batch(g)
    kw = dict(max_events=160, skip_check=False, temp=1.2, top_p=0.97, seed=5)
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='device', **kw)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, scores=True, **kw)
    loop.run()
    at_handoff = {k: t.clone() for k, t in loop.score_tables.items()}
    st0 = loop.state.cpu().numpy().copy()
    out = loop.results(e2i, i2e, 160, False, 5, window='device')
    assert out == plain
    sc = loop.scores(out)
    wl = loop.windowed
    assert len(wl.idx) >= 3
    W, w0 = 48, loop.seq.shape[1]
    st1, seq, segs = wl.state.cpu().numpy(), wl.seq, wl.segs
    err, n = 0.0, 0
    for j, i in enumerate(wl.idx):
        ln0, ln1 = int(st0[i, inf.ACC_S_LEN]), int(st1[j, inf.ACC_S_LEN])
        assert ln0 >= W and ln1 > ln0
        for k in at_handoff:                                                  # the first loop's cells, bit for bit, in the wider rows
            a, b = at_handoff[k][i, :ln0].view(torch.int32), wl.score_tables[k][j, :ln0].view(torch.int32)
            assert torch.equal(a, b), (k, i)
        rank = wl.score_tables['tok_rank'][j].cpu().numpy()
        assert int((rank >= 0).sum()) == int(st1[j, inf.ACC_S_ACCEPTED])       # one cell per accepted draw, both phases
        assert int((rank[ln0:] >= 0).sum()) == int(st1[j, inf.ACC_S_ACCEPTED]) - int(st0[i, inf.ACC_S_ACCEPTED]) > 0
        assert not (rank[ln1:] >= 0).any()
        d = drawn(sc[i])
        assert len(d) == len(out[i]) and d[ln0:].any()
        # after the hand-off: float64 on the logits of the window forward that drew the token (the last W tokens in front of it)
        post = [int(c) for c in np.flatnonzero(d) if c >= ln0]
        assert post[0] <= ln0 + loop.longest_bar + 2                          # the first draw behind the hand-off (an injected bar at most in between)
        for c in sorted(set(post[:4] + post[-4:])):                           # the first cells behind the hand-off and the last of the piece
            with torch.no_grad():
                lg = model(seq[j:j + 1, c - W:c].contiguous(), seg_inp=segs[j:j + 1, c - W:c].contiguous(), keep_last_only=True)
            ref = torch.log_softmax(lg.double().reshape(-1), 0)[int(seq[j, c])].item()
            err = max(err, abs(float(sc[i]['logp'][c]) - ref))
            n += 1
    assert n >= 6
    # streams that never reached the window keep their own rows
    for i in range(len(leads)):
        if i not in wl.idx:
            assert int(drawn(sc[i]).sum()) == int(st0[i, inf.ACC_S_ACCEPTED]) - (1 if st0[i, inf.ACC_S_STATUS] == inf.ACC_DONE else 0)
    print('[measured] past the window, GPT-2 fp32: max |recorded - float64 on the one-row window forward| = %.3e over %d tokens' % (err, n))
    assert err <= ROW_TOL


# ------------------------------------------------------------------------------------------------ 6. best_of by draws
def test_best_by_draws_picks_by_the_recorded_means_and_runs_no_forward(monkeypatch):
    from emo_disentanger_amd import inference as inf, scoring, stage1_inference as s1
    calls = {'s1': 0, 's2': 0}
    real1, real2 = scoring.lead_sheet_candidate_scores, scoring.candidate_scores

    def count1(*a, **k):
        calls['s1'] += 1
        return real1(*a, **k)

    def count2(*a, **k):
        calls['s2'] += 1
        return real2(*a, **k)

    monkeypatch.setattr(scoring, 'lead_sheet_candidate_scores', count1)
    monkeypatch.setattr(scoring, 'candidate_scores', count2)
    m, e2i, i2e = _generator_fixture()
    res, _, picks, sc = s1.generate_lead_sheets(m, e2i, i2e, S1_PRIMERS[:4], best_of=2, best_by='draws', return_scores=True, **S1_KW)
    assert calls['s1'] == 0
    plain, _ = s1.generate_lead_sheets(m, e2i, i2e, [p for p in S1_PRIMERS[:4] for _ in range(2)], **S1_KW)
    for i, p in enumerate(picks):
        means = scoring.draw_scores_mean(p['scores'])
        assert [a != a for a in means] == [not ok(c) for c in p['candidates']]
        assert all(a == b or (a != a and b != b) for a, b in zip(means, p['nll_mean']))
        assert p['chosen'] == scoring.best_of(means)
        if any(x == x for x in means):
            assert p['chosen'] == int(np.nanargmin(means)) and res[i] == p['candidates'][p['chosen']] and sc[i] is p['scores'][p['chosen']]
        assert all(same(c, plain[2 * i + k]) for k, c in enumerate(p['candidates']))
    fwd, _, fpicks = s1.generate_lead_sheets(m, e2i, i2e, S1_PRIMERS[:4], best_of=2, best_by='forward', **S1_KW)
    dflt, _, dpicks = s1.generate_lead_sheets(m, e2i, i2e, S1_PRIMERS[:4], best_of=2, **S1_KW)
    assert calls['s1'] == 2 and [p['chosen'] for p in fpicks] == [p['chosen'] for p in dpicks] and all(same(a, b) for a, b in zip(fwd, dflt))
    assert all('scores' not in p for p in dpicks)

    g, e2i, i2e = _vocab()
    model = _tiny('gpt2', 'fp32')
    lead = [list(b) for b in g['lead']]
    leads, primers = [lead, lead[::-1], lead[:2]], [list(g['primer']), [1, 5, 6], [2, 4, 6]]
    kw = dict(max_events=150, skip_check=False, temp=1.2, top_p=0.97, seed=5)
    res, _, picks, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=2, best_by='draws', return_scores=True, **kw)
    assert calls['s2'] == 0 and len(res) == len(picks) == 3
    for i, p in enumerate(picks):
        means = scoring.draw_scores_mean(p['scores'])
        assert means == p['nll_mean'] and all(x == x for x in means)
        assert p['chosen'] == int(np.argmin(means)) and res[i] == p['candidates'][p['chosen']]
    fwd, _, fpicks = inf.generate_accompaniments(model, e2i, i2e, leads, primers, best_of=2, **kw)
    assert calls['s2'] == 1
    assert [p['candidates'] for p in fpicks] == [p['candidates'] for p in picks]     # the same candidates, ranked by the other figure
