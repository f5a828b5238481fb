"""GPU: window='rebase' — emo_acc_rebase against inference.rebase_plan and a NumPy restatement on handed-off rows, and the re-anchored
continuation end to end on both backbones: the prefix up to the first hand-off, the host grammar on every id, the lead-sheet bars in order,
max_events, the stitched score tables, best_of by draws, slots, and the error of a stream whose bar outgrows the window.  The window is
lowered to 96 tokens and rebase_keep to 48, so every stream is re-anchored at least twice."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
W, KEEP, MAX_EVENTS = 96, 48, 330


def _vocab():
    g = json.load(open(os.path.join(G, 'generate.json')))
    e2i = {e: i for i, e in enumerate(g['events'])}
    return g, e2i, {i: e for e, i in e2i.items()}


_MODELS = {}


def _tiny(kind):
    if kind not in _MODELS:
        from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
        from emo_disentanger_amd.model.music_performer import MusicPerformer
        from oracle.weights import make_state_dict
        g = json.load(open(os.path.join(G, 'generate.json')))
        m = g['model']
        if kind == 'gpt2':
            sd = make_state_dict('gpt2', m['V'], m['L'], m['H'], m['d'], m['dff'], seed=m['seed'], scale=m['scale'])
            mod = MusicGPT2(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], dropout=0.1, use_segment_emb=True, n_segment_types=2, compute_dtype='fp32')
        else:
            sd = make_state_dict('performer', m['V'], m['L'], m['H'], m['d'], m['dff'], favor_feature_dims=32, seed=m['seed'], scale=m['scale'])
            mod = MusicPerformer(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], favor_feature_dims=32, use_segment_emb=True, n_segment_types=2,
                                 compute_dtype='fp32', redraw='fixed')
        # bars of a dozen or two events, far below the window (measured: the Performer's bars at +2.5 are 10 tokens, GPT-2's pass 88)
        sd['dec_out_proj.bias'][g['events'].index('Track_LeadSheet')] += 3.4 if kind == 'gpt2' else 0.4
        mod.load_state_dict(sd)
        _MODELS[kind] = mod.cuda().eval()
    return _MODELS[kind]


def _batch(g):
    """4 streams of 12-bar synthetic lead sheets."""
    lead = [list(b) for b in g['lead']]
    leads = [(lead * 4)[:12], (lead[::-1] * 4)[:12], (lead[1:] + lead[:1]) * 4, [lead[1]] * 12]
    assert all(len(x) == 12 for x in leads)
    return leads, [list(g['primer']), [1, 5, 6], [2, 4, 6], [3, 5, 6]]


KW = dict(max_events=MAX_EVENTS, skip_check=False, temp=1.2, top_p=0.97, seed=5)


def _replay_on_host(inf, e2i, i2e, ids, lead, primer, max_events):
    """Feed the ids to _Stream.offer in order: none is rejected, and the injected bars are the piece's own."""
    s = inf._Stream(e2i, lead, primer, None)
    at = len(s.generated)
    assert ids[:at] == s.generated
    while at < len(ids):
        assert not s.done, at
        assert s.offer(ids[at], e2i, i2e, False, max_events) and not s.stuck, (at, ids[at])
        n = min(len(s.generated), len(ids))
        assert s.generated[at:n] == ids[at:n], at
        at = len(s.generated)
    return s


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_rebase_kernel_matches_the_plan_on_handed_off_rows(kind, monkeypatch):
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', W)
    leads, primers = _batch(g)
    loop = inf.AccompanimentLoop(_tiny(kind), e2i, i2e, leads, primers, scores=True, **KW)
    loop.run()
    rl = inf.RebaseLoop(loop, 5, KEEP)
    assert len(rl.idx) >= 3
    m0, tls, pad, longest = rl.m0, e2i['Track_LeadSheet'], loop.pad, loop.longest_bar
    state0, params0 = rl.state.cpu().numpy().copy(), rl.params.cpu().numpy().copy()
    state0[0, inf.ACC_S_STATUS] = inf.ACC_DONE                 # one row that is not at the window: untouched
    state_d, params_d = torch.from_numpy(state0.copy()).cuda(), torch.from_numpy(params0.copy()).cuda()
    seq0, segs0 = rl.seq_pp[0].cpu().numpy(), rl.segs_pp[0].cpu().numpy()
    sc0 = {k: t.cpu().numpy() for k, t in rl.scores_pp[0].items()}
    width = seq0.shape[1]
    dst_seq, dst_segs = torch.full((m0, width), -7, dtype=torch.int64, device='cuda'), torch.full((m0, width), -7, dtype=torch.int64, device='cuda')
    dst_sc, arch_sc = ops.draw_score_tables(dst_seq), ops.draw_score_tables(rl.arch_tok)
    arch = torch.full_like(rl.arch_tok, -7)
    arch_len = torch.tensor([3] * m0, dtype=torch.int32, device='cuda')            # a cursor that is not at 0
    new_len = torch.full((m0,), -7, dtype=torch.int32, device='cuda')
    running = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.acc_rebase(rl.seq_pp[0], rl.segs_pp[0], state_d, params_d, rl.primer_len, tls, KEEP, W, longest, pad, dst_seq, dst_segs, arch, arch_len,
                   new_len, running, scores=rl.scores_pp[0], dst_scores=dst_sc, arch_scores=arch_sc)
    torch.cuda.synchronize()
    st, pr, nl, al = state_d.cpu().numpy(), params_d.cpu().numpy(), new_len.cpu().numpy(), arch_len.cpu().numpy()
    ds, dg, ar = dst_seq.cpu().numpy(), dst_segs.cpu().numpy(), arch.cpu().numpy()
    went_on = 0
    assert nl[0] == 0 and (st[0] == state0[0]).all() and (ds[0] == -7).all() and al[0] == 3 and (ar[0] == -7).all()
    for j in range(1, m0):
        n, P = int(state0[j, inf.ACC_S_LEN]), len(primers[rl.idx[j]])
        assert n >= W
        plan = inf.rebase_plan(seq0[j], n, P, tls, KEEP, W, longest)
        if plan == inf.ACC_BAR_TOO_LONG:                       # the status alone changes
            want = state0[j].copy()
            want[inf.ACC_S_STATUS] = inf.ACC_BAR_TOO_LONG
            assert (st[j] == want).all() and (pr[j] == params0[j]).all() and nl[j] == 0 and al[j] == 3 and (ds[j] == -7).all()
            continue
        went_on += 1
        b, want_len = plan
        assert seq0[j, b] == tls and want_len == nl[j] <= W - longest - 2       # (at most KEEP, or the fallback to the last bar)
        ctx = list(seq0[j, :P]) + list(seq0[j, b:n])
        assert ds[j, :want_len].tolist() == ctx and (ds[j, want_len:] == pad).all()
        assert dg[j, :want_len].tolist() == list(segs0[j, :P]) + list(segs0[j, b:n]) and (dg[j, want_len:] == 1).all()
        assert al[j] == 3 + b - P and ar[j, 3:al[j]].tolist() == list(seq0[j, P:b]) and (ar[j, al[j]:] == -7).all()
        want = state0[j].copy()
        want[[inf.ACC_S_STATUS, inf.ACC_S_LEN, inf.ACC_S_CONSUMED, inf.ACC_S_DRAWS]] = inf.ACC_RUNNING, want_len, want_len, 0
        assert (st[j] == want).all()
        wp = params0[j].copy()
        wp[inf.ACC_P_MAX_EVENTS] = inf.rebase_max_events(params0[j, inf.ACC_P_MAX_EVENTS], b, P)
        assert (pr[j] == wp).all()
        for k in sc0:
            d, a = dst_sc[k].cpu().numpy(), arch_sc[k].cpu().numpy()
            src = np.concatenate([sc0[k][j, :P], sc0[k][j, b:n]])
            np.testing.assert_array_equal(d[j, :want_len], src)
            np.testing.assert_array_equal(a[j, 3:al[j]], sc0[k][j, P:b])
            assert (d[j, want_len:] == -1).all() if k == 'tok_rank' else np.isnan(d[j, want_len:]).all()
    assert int(running.item()) == went_on >= 2


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_rebase_continuation_obeys_the_grammar_and_keeps_the_prefix(kind, monkeypatch):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', W)
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    model = _tiny(kind)
    leads, primers = _batch(g)
    host, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='host', **KW)
    got, _, sc = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='rebase', rebase_keep=KEEP, return_scores=True, **KW)
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='rebase', rebase_keep=KEEP, use_graph=False, **KW)
    assert all(isinstance(x, list) for x in got), got
    assert plain == got                                        # graphs or not, scores or not: the same ids
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, scores=True, **KW)
    loop.run()
    out = loop.results(e2i, i2e, MAX_EVENTS, False, 5, window='rebase', rebase_keep=KEEP)
    assert out == got
    rl = loop.windowed
    print('rebase %s: phases %d, per stream %s, lengths %s, dropped %s' % (kind, rl.phases, rl.rebased, [len(x) for x in got], rl.arch_len.tolist()))
    assert isinstance(rl, inf.RebaseLoop) and rl.phases >= 2 and len(rl.idx) == 4
    assert min(rl.rebased) >= 2                                # every stream was re-anchored at least twice
    hand = loop.state[:, inf.ACC_S_LEN].cpu().tolist()
    tls, tf = e2i['Track_LeadSheet'], e2i['Track_Full']
    for i, ids in enumerate(got):
        assert isinstance(ids, list) and len(ids) > W and len(ids) <= MAX_EVENTS
        assert ids[:hand[i]] == host[i][:hand[i]] and hand[i] >= W          # every id up to the first hand-off is window='host''s
        s = _replay_on_host(inf, e2i, i2e, ids, leads[i], primers[i], MAX_EVENTS)
        starts = [j for j, w in enumerate(ids) if w == tls]
        assert 1 <= len(starts) <= 12 and s.generated_bars == len(starts) - 1
        for k, j in enumerate(starts):                         # the lead-sheet bars, in order
            assert ids[j + 1:j + 2 + len(leads[i][k])] == (leads[i][k] + [tf])[:len(ids) - j - 1], (i, k)
        # scores: sentinels exactly where tokens were given, finite where drawn, across the stitches
        given = np.zeros(len(ids), bool)
        given[:len(primers[i])] = True
        for k, j in enumerate(starts):
            given[j + 1:j + 2 + len(leads[i][k])] = True
        given[starts[0]] = True                                # the first Track_LeadSheet opens the prompt; every later one was drawn
        lp, rk, en = sc[i]['logp'], sc[i]['rank'], sc[i]['entropy']
        assert len(lp) == len(rk) == len(en) == len(ids)
        assert np.isnan(lp[given]).all() and (rk[given] == -1).all() and np.isnan(en[given]).all()
        assert np.isfinite(lp[~given]).all() and (rk[~given] >= 0).all() and np.isfinite(en[~given]).all() and (lp[~given] <= 0).all()


def test_rebase_kernel_takes_every_branch_on_hand_built_rows():
    """Rows built by hand, one per branch of emo_acc_rebase: the smallest bar start that fits `keep`; no bar start fits and the last one is
    taken (exactly at the bound window - longest_bar - 2); the same row one token longer: a bar longer than the window; a row without any bar
    start; a row that is not at the window.  Every row starts from a cursor of its own in the archive."""
    from emo_disentanger_amd import inference as inf, ops
    TLS, TF, X, PAD, Wk, keep, longest, width = 7, 8, 3, 39, 64, 24, 2, 80
    bar = lambda body: [TLS, X, X, TF] + [X] * body      # noqa: E731
    rows = [[1, 2, 5] + bar(6) * 6 + bar(4),                   # P 3, n 71: bar starts 3, 13, .., 53, 63: the cut at 53 leaves 21 <= 24
            [1, 2] + bar(6) + bar(54),                         # P 2, n 70: the last bar start 12 leaves 60 = 64 - 2 - 2: the fallback, exactly
            [1, 2] + bar(6) + bar(55),                         # one token more: 61 > 60: a bar longer than the window
            [1, 2, 5] + [X] * 67,                              # no bar start behind the primer
            [1, 2, 5] + bar(6) * 6]                            # DONE: not touched
    P = [3, 2, 2, 3, 3]
    status = [inf.ACC_WINDOW] * 4 + [inf.ACC_DONE]
    cursor = [0, 5, 2, 1, 4]
    n = len(rows)
    seq, segs = np.full((n, width), PAD, np.int64), np.ones((n, width), np.int64)
    state, params = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
    for j, r in enumerate(rows):
        seq[j, :len(r)] = r
        segs[j, :len(r)] = [int(i >= P[j] and w != TLS) for i, w in enumerate(r)]
        state[j] = [status[j], len(r), len(r) - 1, 3 + j, 5, 2, 40 + j, 30 + j]
        params[j] = [12, 300 + j, 0, 0, 12, 0, 0, 0]
    T = lambda a: torch.from_numpy(a.copy()).cuda()           # noqa: E731
    seq_d, segs_d, state_d, params_d = T(seq), T(segs), T(state), T(params)
    dst_seq, dst_segs = torch.full((n, width), -7, dtype=torch.int64, device='cuda'), torch.full((n, width), -7, dtype=torch.int64, device='cuda')
    arch = torch.full((n, 100), -7, dtype=torch.int64, device='cuda')
    arch_len, new_len = T(np.array(cursor, np.int32)), torch.full((n,), -7, dtype=torch.int32, device='cuda')
    running = torch.zeros(1, dtype=torch.int32, device='cuda')
    ops.acc_rebase(seq_d, segs_d, state_d, params_d, T(np.array(P, np.int32)), TLS, keep, Wk, longest, PAD, dst_seq, dst_segs, arch, arch_len, new_len,
                   running)
    torch.cuda.synchronize()
    st, pr, nl, al, ds, dg, ar = (x.cpu().numpy() for x in (state_d, params_d, new_len, arch_len, dst_seq, dst_segs, arch))
    plans = [inf.rebase_plan(rows[j], len(rows[j]), P[j], TLS, keep, Wk, longest) for j in range(4)]
    assert plans == [(53, 21), (12, 60), inf.ACC_BAR_TOO_LONG, inf.ACC_BAR_TOO_LONG]
    for j in range(n):
        if j < 2:
            b, ln = plans[j]
            assert nl[j] == ln and ds[j, :ln].tolist() == rows[j][:P[j]] + rows[j][b:] and (ds[j, ln:] == PAD).all()
            assert dg[j, :ln].tolist() == list(segs[j, :P[j]]) + list(segs[j, b:len(rows[j])]) and (dg[j, ln:] == 1).all()
            assert al[j] == cursor[j] + b - P[j] and ar[j, cursor[j]:al[j]].tolist() == rows[j][P[j]:b]
            assert (ar[j, :cursor[j]] == -7).all() and (ar[j, al[j]:] == -7).all()
            assert st[j].tolist() == [inf.ACC_RUNNING, ln, ln, 3 + j, 5, 2, 0, 30 + j]
            assert pr[j].tolist() == [12, 300 + j - (b - P[j]), 0, 0, 12, 0, 0, 0]
        else:
            want = state[j].copy()
            if j < 4:
                want[inf.ACC_S_STATUS] = inf.ACC_BAR_TOO_LONG
            assert (st[j] == want).all() and (pr[j] == params[j]).all() and nl[j] == 0 and al[j] == cursor[j]
            assert (ds[j] == -7).all() and (dg[j] == -7).all() and (ar[j] == -7).all()
    assert int(running.item()) == 2


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_full_shape_rebase_runs_the_one_launch_step(kind):
    """d 512, 12 layers, bf16, the 2048-token window: the phases run on the one-launch engines (zeroed padding rows, per-row positions, GPT-2's
    key counts from them), and the pieces obey the grammar well past the window."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('stage2_window_shapes', os.path.join(os.path.dirname(__file__), 'test_gpu_stage2_window.py'))
    sw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sw)
    from emo_disentanger_amd import inference as inf
    e2i, i2e = sw._full_vocab()
    leads, primers = sw._full_batch(e2i, n=6, bars=260)        # about 17 tokens a bar: pieces that fill the window, then half of it twice more
    model = sw._full_model(kind)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, seed=4, max_events=4200, temp=1.2, top_p=0.9)
    loop.run()
    out = loop.results(e2i, i2e, 4200, False, 4, window='rebase')
    rl = loop.windowed
    assert isinstance(rl, inf.RebaseLoop) and rl.eng.persist is not None and rl.persistent and rl.keep == 1024
    assert len(rl.idx) >= 4 and rl.phases >= 1 and max(rl.rebased) >= 2, (rl.idx, rl.phases, rl.rebased)
    for i, (ids, ld, pr) in enumerate(zip(out, leads, primers)):
        sw._grammar_ok(inf, e2i, i2e, ids, ld, pr)
        if i in rl.idx:
            assert len(ids) > 2048 + 200, (i, len(ids))


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_rebase_with_best_of_by_draws_slots_and_a_bar_longer_than_the_window(kind, monkeypatch):
    from emo_disentanger_amd import _lib, inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', W)
    model = _tiny(kind)
    leads, primers = _batch(g)
    out, _, picks = inf.generate_accompaniments(model, e2i, i2e, leads[:2], primers[:2], window='rebase', rebase_keep=KEEP, best_of=2, best_by='draws', **KW)
    assert len(out) == 2 and len(picks) == 2
    for ids, p, ld, pr in zip(out, picks, leads, primers):
        assert p['chosen'] in (0, 1) and ids == p['candidates'][p['chosen']] and len(ids) > W
        assert np.isfinite(p['nll_mean'][p['chosen']])
        _replay_on_host(inf, e2i, i2e, ids, ld, pr, MAX_EVENTS)
    # 4 jobs through 2 slots: the jobs that leave the queue at the window are finished by the rebase phases
    q, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='rebase', rebase_keep=KEEP, slots=2, **KW)
    assert len(q) == 4
    for ids, ld, pr in zip(q, leads, primers):
        assert isinstance(ids, list) and len(ids) > W
        _replay_on_host(inf, e2i, i2e, ids, ld, pr, MAX_EVENTS)
    # stream 1 may never draw Track_LeadSheet: its bar outgrows the window, the others finish
    bans = [None, [e2i['Track_LeadSheet']], None, None]
    e, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='rebase', rebase_keep=KEEP, banned=bans, **KW)
    assert isinstance(e[1], _lib.EmoError) and 'a bar longer than the window' in str(e[1])
    for i in (0, 2, 3):
        assert isinstance(e[i], list) and len(e[i]) > W
        _replay_on_host(inf, e2i, i2e, e[i], leads[i], primers[i], MAX_EVENTS)
