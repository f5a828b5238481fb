"""GPU: stage-2 streams past the max_dec_inp_len window on the device — the windowed step emo_acc_window_step against a host restatement on
_Stream.offer, the batched WindowedLoop against the host grammar on the same draws (same batched forward, poll interval and compaction rule),
its tie to _resume_windowed at one stream, the prefix / default guarantees of generate_accompaniments(window=...), compaction, the full shape
and the --window command line."""
import copy
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')


def _vocab():
    g = json.load(open(os.path.join(G, 'generate.json')))
    e2i = {e: i for i, e in enumerate(g['events'])}
    return g, e2i, {i: e for e, i in e2i.items()}


def _tiny(kind, dtype, tls_bias=0.0):
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    from oracle.weights import make_state_dict
    g = json.load(open(os.path.join(G, 'generate.json')))
    m = g['model']
    if kind == 'gpt2':
        sd = make_state_dict('gpt2', m['V'], m['L'], m['H'], m['d'], m['dff'], seed=m['seed'], scale=m['scale'])
        mod = MusicGPT2(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], dropout=0.1, use_segment_emb=True, n_segment_types=2, compute_dtype=dtype)
    else:
        sd = make_state_dict('performer', m['V'], m['L'], m['H'], m['d'], m['dff'], favor_feature_dims=32, seed=m['seed'], scale=m['scale'])
        mod = MusicPerformer(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], favor_feature_dims=32, use_segment_emb=True, n_segment_types=2,
                             compute_dtype=dtype, redraw='fixed')
    if tls_bias:
        sd['dec_out_proj.bias'][g['events'].index('Track_LeadSheet')] += tls_bias      # bars end soon
    mod.load_state_dict(sd)
    return mod.cuda().eval()


def _grammar_ok(inf, e2i, i2e, ids, lead, primer):
    """The checks of test_full_shape_pieces_obey_the_grammar on one piece: every Track_LeadSheet is followed by its bar and Track_Full, Beats
    ascend inside a bar, no PAD."""
    tls, tf = e2i['Track_LeadSheet'], e2i['Track_Full']
    assert isinstance(ids, list), ids
    assert ids[:len(primer)] == primer and e2i['PAD_None'] not in ids
    starts = [j for j, w in enumerate(ids) if w == tls]
    assert 1 <= len(starts) <= len(lead)
    for k, j in enumerate(starts):
        assert ids[j + 1:j + 2 + len(lead[k])] == lead[k] + [tf], k
        body = ids[j + 2 + len(lead[k]):(starts[k + 1] if k + 1 < len(starts) else len(ids))]
        beats = [inf.beat_position(i2e[w]) for w in body if 'Beat' in i2e[w]]
        assert beats == sorted(beats), (k, beats)
    return len(starts) == len(lead)


# ------------------------------------------------------------------------------------------------ the kernel, launch by launch
class HostWin:
    """Host restatement of one stream of emo_acc_window_step on _Stream.offer."""

    def __init__(self, inf, e2i, i2e, lead, primer, max_bars, max_events, skip_check, W, width, filler, done=False):
        self.inf, self.e2i, self.i2e = inf, e2i, i2e
        self.s = inf._Stream(e2i, lead, primer, max_bars)
        while len(self.s.generated) < W:                      # the in-window phase: plain events up to the handoff
            assert self.s.offer(filler, e2i, i2e, skip_check, 10 ** 6) and not self.s.done
        self.s.consumed = len(self.s.generated) - 1
        self.max_events, self.skip, self.W, self.width = max_events, skip_check, W, width
        self.status = inf.ACC_DONE if done else inf.ACC_RUNNING
        self.draws = self.accepted = 0
        self.win = None                                       # (tokens, segments) of the stream's window row, once written

    def offer(self, w, n_u):
        """One draw through the grammar -> True when the launch draws again."""
        inf = self.inf
        self.draws += 1
        t = copy.deepcopy(self.s)
        ok = t.offer(w, self.e2i, self.i2e, self.skip, self.max_events)
        if len(t.generated) > self.width:                     # the accepted tokens do not fit the row: nothing is written (the Beat check ran)
            if not self.skip and 'Beat' in self.i2e[w]:
                self.s.cur_pos, self.s.failed_cnt = t.cur_pos, t.failed_cnt
            self.status = inf.ACC_OVERFLOW
            return False
        self.s = t
        if t.stuck:
            self.status = inf.ACC_STUCK
        elif ok:
            self.accepted += 1
            if t.done:
                self.status = inf.ACC_DONE
            else:
                self.win = (t.generated[-self.W:], t.seg[-self.W:])
        elif self.draws >= n_u:
            self.status = inf.ACC_OUT_OF_DRAWS
        else:
            return True
        return False

    def state(self):
        inf, s = self.inf, self.s
        return {inf.ACC_S_STATUS: self.status, inf.ACC_S_LEN: len(s.generated), inf.ACC_S_CONSUMED: s.consumed, inf.ACC_S_BARS: s.generated_bars,
                inf.ACC_S_CUR_POS: s.cur_pos, inf.ACC_S_FAILED: s.failed_cnt, inf.ACC_S_DRAWS: self.draws, inf.ACC_S_ACCEPTED: self.accepted}


B = lambda k: 'Beat_%d' % k      # noqa: E731
FILL = 'Note_Duration_4'
# per stream: lead sheet (bar indices into generate.json's lead), primer, max_bars, max_events, skip_check, starts finished, and per launch the
# boosted words (None: the launch draws from the random logits alone)
WIN_UNIT = [
    # a Beat going backwards: rejected, redrawn in the SAME launch; Track_LeadSheet mid-piece (bar injection, cur_pos reset), then at the last
    # bar -> DONE
    ([0, 1], [0, 4, 6], None, 10 ** 4, False, False, [[B(5)], [B(2), B(8)], ['Note_Octave_4'], ['Track_LeadSheet'], [B(0)], ['Track_LeadSheet']]),
    # 256 Beats in a row below the position -> STUCK inside one launch
    ([0, 1, 2], [1, 5, 6], None, 10 ** 4, False, False, [[B(6)], [B(1)]]),
    # PAD and a premature EOS (rejected, not counted), then EOS at the last bar -> DONE
    ([0, 2], [0, 4, 6], None, 10 ** 4, False, False,
     [['Chord_I_M', 'PAD_None'], ['Note_Degree_1', 'EOS_None'], ['Track_LeadSheet'], [B(3)], ['EOS_None']]),
    # finished before the first launch: never drawn for, its window row never written
    ([0, 1], [2, 4, 6], None, 10 ** 4, False, True, []),
    # plain events until the row is full -> OVERFLOW
    ([0, 1, 2], [2, 5, 6], None, 10 ** 4, False, False, [['Note_Velocity_60']] * 48),
    # max_events a few tokens past the handoff
    ([0, 1, 2], [2, 4, 6], None, 27, False, False, [['Note_Octave_4'], [B(1)], ['Note_Degree_1'], ['Chord_V_M'], ['Chord_I_M']]),
    # skip_check: a Beat below the position is accepted
    ([1, 0], [3, 5, 6], None, 10 ** 4, True, False, [[B(7)], [B(2)], [B(0)], ['Track_LeadSheet'], ['Track_LeadSheet']]),
    # random logits alone, whatever they give
    ([0, 1, 2, 0, 1], [0, 4, 6], None, 36, False, False, [None] * 64),
    ([2, 1, 0, 2, 1], [1, 5, 6], None, 36, True, False, [None] * 64),
]
W_WIN, NU_WIN, WIDTH_WIN = 24, 300, 64


def test_window_kernel_matches_the_host_grammar_launch_by_launch():
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    V, n, dev = len(i2e), len(WIN_UNIT), 'cuda'
    leads = [[list(g['lead'][j]) for j in u[0]] for u in WIN_UNIT]
    flags, beat = inf.acc_event_tables(i2e, V)
    toks, offs, bar0, nbars, longest = inf.pack_lead_sheets(leads)
    width = WIDTH_WIN
    assert width >= W_WIN + 2 * (longest + 2)
    hosts = [HostWin(inf, e2i, i2e, ld, u[1], u[2], u[3], u[4], W_WIN, width, e2i[FILL], done=u[5]) for u, ld in zip(WIN_UNIT, leads)]
    rs = np.random.RandomState(7)
    U = rs.uniform(0.05, 0.45, size=(NU_WIN, n)).astype(np.float32)
    U[:, 7:] = rs.uniform(0.0, 1.0, size=(NU_WIN, n - 7))
    # two boosted words are equally likely: u < 0.5 picks the lower id, u >= 0.5 the higher (as in the in-window kernel's test)
    U[1, 0], U[2, 0] = 0.2, 0.8
    U[0, 2], U[1, 2], U[2, 2], U[3, 2] = 0.8, 0.2, 0.8, 0.2
    seq, segs = np.zeros((n, width), np.int64), np.zeros((n, width), np.int64)
    params, state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
    for i, (h, u) in enumerate(zip(hosts, WIN_UNIT)):
        k = len(h.s.generated)
        assert W_WIN <= k <= width
        seq[i, :k], segs[i, :k] = h.s.generated, h.s.seg
        params[i, :5] = h.s.target_bars, u[3], u[4], bar0[i], nbars[i]
        for w, v in h.state().items():
            state[i, w] = v
    T = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    seq_d, segs_d, params_d, state_d, U_d = T(seq), T(segs), T(params), T(state), T(U)
    ev_flags, ev_beat, lead_tok, lead_off = T(flags), T(beat), T(toks), T(offs)
    running = torch.tensor([sum(h.status == inf.ACC_RUNNING for h in hosts)], dtype=torch.int32, device=dev)
    order = list(range(n))[::-1]                   # batch row b holds stream order[b]
    rows = torch.tensor(order, dtype=torch.int32, device=dev)
    win_tok = torch.full((n, W_WIN), -7, dtype=torch.long, device=dev)
    win_seg = torch.full((n, W_WIN), -7, dtype=torch.long, device=dev)
    launches, steps = [0] * n, 0
    while any(h.status == inf.ACC_RUNNING for h in hosts):
        logits = rs.randn(n, V).astype(np.float32) * 2.0
        for b, i in enumerate(order):
            if hosts[i].status == inf.ACC_RUNNING:
                c = WIN_UNIT[i][6][launches[i]]
                launches[i] += 1
                if c is not None:
                    logits[b, [e2i[w] for w in c]] = 60.0         # one or two words far above the rest: the nucleus keeps exactly those
        logits_d = T(logits)
        ops.acc_window_step(logits_d, 1.2, 0.9, U_d, rows, ev_flags, ev_beat, lead_tok, lead_off, params_d, state_d, seq_d, segs_d, W_WIN,
                            e2i['Track_Full'], win_tok, win_seg, running)
        want = [b for b, i in enumerate(order) if hosts[i].status == inf.ACC_RUNNING]
        while want:                                # one draw for every stream that wants one, again for the rejected ones
            u = torch.tensor([float(U[min(hosts[i].draws, NU_WIN - 1), i]) for i in order], dtype=torch.float32, device=dev)
            words = ops.sample_nucleus(logits_d, 1.2, 0.9, u).cpu().tolist()
            want = [b for b in want if hosts[order[b]].offer(words[b], NU_WIN)]
        st, sq, sg, wt, ws = (x.cpu().numpy() for x in (state_d, seq_d, segs_d, win_tok, win_seg))
        for b, i in enumerate(order):
            h = hosts[i]
            for k, v in h.state().items():
                assert st[i, k] == v, (steps, i, k, st[i].tolist())
            assert sq[i, :len(h.s.generated)].tolist() == h.s.generated, (steps, i)
            assert sg[i, :len(h.s.seg)].tolist() == h.s.seg, (steps, i)
            if h.win is None:
                assert (wt[b] == -7).all() and (ws[b] == -7).all(), (steps, i)
            else:
                assert (wt[b].tolist(), ws[b].tolist()) == h.win, (steps, i)
        assert int(running.item()) == sum(h.status == inf.ACC_RUNNING for h in hosts)
        steps += 1
        assert steps < 200
    want = [inf.ACC_DONE, inf.ACC_STUCK, inf.ACC_DONE, inf.ACC_DONE, inf.ACC_OVERFLOW, inf.ACC_DONE, inf.ACC_DONE]
    assert [h.status for h in hosts[:7]] == want
    assert launches[:7] == [6, 2, 5, 0, width - W_WIN + 1, 4, 5]                # every scripted launch was used, nothing more
    assert hosts[0].draws == 7 and hosts[1].draws == 257 and hosts[2].draws == 7
    assert hosts[0].s.generated_bars == 2 and hosts[3].win is None and hosts[3].draws == 0
    assert len(hosts[4].s.generated) == width and hosts[4].draws == width - W_WIN + 1 and len(hosts[5].s.generated) == 28
    assert all(h.status in (inf.ACC_DONE, inf.ACC_STUCK, inf.ACC_OVERFLOW) for h in hosts[7:])
    assert hosts[7].accepted >= 3 and hosts[8].accepted >= 3


def test_a_prepared_window_block_reused_and_compacted_equals_the_one_shot_wrapper():
    # three streams at the handoff: 0 finished before the first launch, 1 drawing from random logits, 2 accepting four words and then drawing PAD
    # until its table of 8 uniforms is used up (OUT_OF_DRAWS inside its fifth launch).  The batch is m = 2 rows, rows = [2, 0]; after three
    # steps it is compacted to rows = [2] through the setter, which rewrites n_rows and rows in place (what WindowedLoop._set_rows does).  A
    # GrammarStep filled once leaves, word for word, what ops.acc_window_step (a fresh block per call) leaves on its own copies of the tensors.
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    pick = [WIN_UNIT[3], WIN_UNIT[7], WIN_UNIT[4]]
    V, n, dev = len(i2e), len(pick), 'cuda'
    leads = [[list(g['lead'][j]) for j in u[0]] for u in pick]
    flags, beat = inf.acc_event_tables(i2e, V)
    toks, offs, bar0, nbars, longest = inf.pack_lead_sheets(leads)
    hosts = [HostWin(inf, e2i, i2e, ld, u[1], u[2], u[3], u[4], W_WIN, WIDTH_WIN, e2i[FILL], done=u[5]) for u, ld in zip(pick, leads)]
    seq, segs = np.zeros((n, WIDTH_WIN), np.int64), np.zeros((n, WIDTH_WIN), np.int64)
    params, state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
    for i, (h, u) in enumerate(zip(hosts, pick)):
        k = len(h.s.generated)
        seq[i, :k], segs[i, :k] = h.s.generated, h.s.seg
        params[i, :5] = h.s.target_bars, u[3], u[4], bar0[i], nbars[i]
        for w, v in h.state().items():
            state[i, w] = v
    T = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    shared = dict(u_steps=torch.rand(8, n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)), ev_flags=T(flags), ev_beat=T(beat),
                  lead_tok=T(toks), lead_off=T(offs), params=T(params))
    fresh = lambda: dict(state=T(state), seq=T(seq), segs=T(segs), win_tok=torch.full((2, W_WIN), -7, dtype=torch.long, device=dev),      # noqa: E731
                         win_seg=torch.full((2, W_WIN), -7, dtype=torch.long, device=dev), running=torch.tensor([2], dtype=torch.int32, device=dev))
    one, blk = fresh(), fresh()
    logits = torch.randn(6, 2, V, device=dev, generator=torch.Generator(device=dev).manual_seed(6)) * 2.0
    logits[:3, 0, e2i['Note_Velocity_60']] = 60.0
    logits[3, 0, e2i['Chord_I_M']] = 60.0
    logits[4:, 0, e2i['PAD_None']] = 60.0
    lg = torch.empty(2, V, device=dev)
    tf = e2i['Track_Full']
    rows2, rows1 = (torch.tensor(r, dtype=torch.int32, device=dev) for r in ([2, 0], [2]))
    args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC_WINDOW), {}
    ops.block_set(args, held, n_rows=2, n_token=V, ld_u=n, temperature=1.2, top_p=0.9, window=W_WIN, track_full=tf, logits=lg, rows=rows2, **shared, **blk)
    for t in range(6):
        m, rows = (2, rows2) if t < 3 else (1, rows1)
        if t == 3:
            ops.block_set(args, held, n_rows=1, rows=rows1)
            assert args.n_rows == 1 and args.rows == rows1.data_ptr() and args.logits == lg.data_ptr() and args.win_tok == blk['win_tok'].data_ptr()
        lg.copy_(logits[t])
        ops.acc_window_step(lg[:m], 1.2, 0.9, shared['u_steps'], rows, shared['ev_flags'], shared['ev_beat'], shared['lead_tok'], shared['lead_off'],
                            shared['params'], one['state'], one['seq'], one['segs'], W_WIN, tf, one['win_tok'][:m], one['win_seg'][:m], one['running'])
        ops.grammar_step(args)
        for k in one:
            assert torch.equal(one[k], blk[k]), (t, k, one[k].tolist(), blk[k].tolist())
    st = blk['state'].cpu().numpy()
    assert st[:, inf.ACC_S_STATUS].tolist() == [inf.ACC_DONE, inf.ACC_RUNNING, inf.ACC_OUT_OF_DRAWS] and int(blk['running'].item()) == 1
    assert st[:, inf.ACC_S_DRAWS].tolist() == [0, 0, 8] and st[2, inf.ACC_S_ACCEPTED] == 4
    assert (blk['win_tok'][1] == -7).all() and (blk['win_tok'][0] >= 0).all()        # the finished stream's row was never written


# ------------------------------------------------------------------------------------------------ the loop against the host grammar
def _host_window_loop(inf, model, e2i, i2e, loop, wl, max_events, skip_check):
    """The windowed phase restated on the host: the SAME batched forward on the same rows, ops.sample_nucleus on each stream's own column of
    the windowed table at its own draw counter, _Stream.offer, the same poll interval and compaction rule.  loop: the finished in-window
    loop; wl: a WindowedLoop built on it (for its table, stream order and poll interval; not run).
    -> (streams, status per stream, row count of every step)."""
    from emo_disentanger_amd import ops
    W, U, k, dev = loop.W, wl.U, wl.k, loop.dev
    st = [copy.deepcopy(loop.handed_off(i)) for i in wl.idx]
    m0 = len(st)
    status, draws = [inf.ACC_RUNNING] * m0, [0] * m0
    kw = {'attn_kwargs': {'omit_feature_map_draw': True}} if model.kind == 'performer' else {}
    rows = list(range(m0))
    win = [(st[j].generated[-W:], st[j].seg[-W:]) for j in rows]
    batch_rows = []
    with torch.no_grad():
        while True:
            for _ in range(k):
                tok = torch.tensor([w[0] for w in win], device=dev)
                seg = torch.tensor([w[1] for w in win], device=dev)
                logits = model(tok, seg_inp=seg, keep_last_only=True, **kw).float().contiguous()
                want = [b for b, j in enumerate(rows) if status[j] == inf.ACC_RUNNING]
                while want:
                    u = torch.stack([U[min(draws[j], U.shape[0] - 1), j] for j in rows]).contiguous()
                    words = ops.sample_nucleus(logits, loop.temp, loop.top_p, u).cpu().tolist()
                    again = []
                    for b in want:
                        j = rows[b]
                        if draws[j] >= U.shape[0]:
                            status[j] = inf.ACC_OUT_OF_DRAWS
                            continue
                        draws[j] += 1
                        ok = st[j].offer(words[b], e2i, i2e, skip_check, max_events)
                        if st[j].stuck:
                            status[j] = inf.ACC_STUCK
                        elif ok and st[j].done:
                            status[j] = inf.ACC_DONE
                        elif ok:
                            win[b] = (st[j].generated[-W:], st[j].seg[-W:])
                        else:
                            again.append(b)
                    want = again
                batch_rows.append(len(rows))
            live = [status[j] == inf.ACC_RUNNING for j in rows]
            if not any(live):
                break
            keep = inf.window_compaction(live)
            if len(keep) < len(rows):
                rows = [rows[p] for p in keep]
                win = [(st[j].generated[-W:], st[j].seg[-W:]) for j in rows]
    return st, status, batch_rows


def _tiny_batch(g):
    lead = [list(b) for b in g['lead']]
    leads = [lead * 4, lead, lead[::-1] * 3, [lead[1]] * 9, lead * 3, lead * 2 + lead[:1]]
    primers = [list(g['primer']), [1, 5, 6], [2, 4, 6], [2, 4], [3, 5, 6], [0, 4, 6, 26, 27]]
    return leads, primers


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('skip_check', [False, True])
def test_windowed_loop_equals_host_grammar_on_the_same_draws(kind, dtype, skip_check, monkeypatch):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    model = _tiny(kind, dtype)
    leads, primers = _tiny_batch(g)
    kw = dict(max_events=160, skip_check=skip_check, temp=1.2, top_p=0.97, seed=5)
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, use_graph=True, window='device', **kw)
    eager, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, use_graph=False, window='device', **kw)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
    loop.run()
    wl = inf.WindowedLoop(loop, 5)
    assert wl.k == 4 and len(wl.idx) >= 3                    # several streams cross the window
    st, status, batch_rows = _host_window_loop(inf, model, e2i, i2e, loop, wl, 160, skip_check)
    assert all(x in (inf.ACC_DONE, inf.ACC_STUCK) for x in status)
    for j, i in enumerate(wl.idx):
        assert got[i] == st[j].result(), (i, len(got[i]), len(st[j].result()))
        assert len(got[i]) >= 48
    assert eager == got
    wl.run()                                                  # the loop object itself: same ids, and the schedule of the restatement
    assert wl.results() == [s.result() for s in st]
    assert wl.batch_rows == batch_rows


# ------------------------------------------------------------------------------------------------ tie to the reference-pinned path
@pytest.mark.parametrize('kind', ['gpt2', 'performer'])
def test_one_stream_equals_resume_windowed_on_the_same_draws(kind, monkeypatch):
    """n = 1: the batched forward IS the call _resume_windowed makes, so the device continuation must equal _resume_windowed itself, driven by a
    sampler that draws with ops.sample_nucleus from the logits of that call and the stream's column of the windowed table, in order."""
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    model = _tiny(kind, 'fp32')
    lead = [list(b) for b in g['lead']]
    leads, primers = [lead * 4], [list(g['primer'])]
    kw = dict(max_events=200, skip_check=False, temp=1.2, top_p=0.97, seed=9)
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='device', **kw)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
    loop.run()
    assert loop.state[0, inf.ACC_S_STATUS].item() == inf.ACC_WINDOW
    wl = inf.WindowedLoop(loop, 9)
    s = loop.handed_off(0)
    handoff = len(s.generated)
    seen, d = {}, [0]
    hook = model.register_forward_hook(lambda mod, args, out: seen.__setitem__('logits', out.detach().float().reshape(1, -1).contiguous()))

    def sampler(probs):
        u = wl.U[d[0], 0].reshape(1).contiguous()
        d[0] += 1
        return int(ops.sample_nucleus(seen['logits'], 1.2, 0.97, u).item())

    try:
        rest = inf._resume_windowed(model, e2i, i2e, s, 200, False, 1.2, None, sampler)
    finally:
        hook.remove()
    assert got[0] == rest
    assert len(rest) > handoff >= 48 and d[0] > 0


# ------------------------------------------------------------------------------------------------ prefix and default
def test_device_window_keeps_the_prefix_and_host_stays_the_default(monkeypatch):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    model = _tiny('gpt2', 'fp32', tls_bias=6.0)                # short bars: a one-bar piece ends long before the window
    lead = [list(b) for b in g['lead']]
    leads, primers = [lead * 4, lead[:1], lead * 3, lead[1:2]], [list(g['primer']), [1, 5, 6], [2, 4, 6], [3, 5, 6]]
    kw = dict(max_events=300, skip_check=False, temp=1.2, top_p=0.97, seed=9)
    plain, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **kw)
    host, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='host', **kw)
    device, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='device', **kw)
    assert host == plain
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
    loop.run()
    state = loop.state.cpu().numpy()
    crossed = [i for i in range(len(leads)) if state[i, inf.ACC_S_STATUS] == inf.ACC_WINDOW]
    assert crossed and len(crossed) < len(leads)
    for i in range(len(leads)):
        if i in crossed:
            ln = int(state[i, inf.ACC_S_LEN])
            assert ln >= 48 and device[i][:ln] == host[i][:ln] == loop.seq[i, :ln].cpu().tolist()
            assert len(device[i]) >= ln
        else:
            assert device[i] == host[i]
    with pytest.raises(ValueError):
        inf.generate_accompaniments(model, e2i, i2e, leads, primers, window='bogus', **kw)


# ------------------------------------------------------------------------------------------------ compaction
def test_compaction_shrinks_the_batch_and_keeps_the_pieces(monkeypatch):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    monkeypatch.setenv('EMO_GEN_GRAPH_STEPS', '4')
    model = _tiny('gpt2', 'fp32', tls_bias=6.0)
    lead = [list(b) for b in g['lead']]
    leads = [lead * 3, lead * 16, lead * 3, lead[::-1] * 3, lead * 3, lead[::-1] * 3]        # one long piece among five short ones
    primers = [list(g['primer']), [1, 5, 6], [2, 4, 6], [3, 5, 6], [0, 5, 6], [1, 4, 6]]
    kw = dict(max_events=4000, skip_check=False, temp=1.2, top_p=0.97, seed=3)
    runs = []
    for _ in range(2):
        loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
        loop.run()
        out = loop.results(e2i, i2e, 4000, False, 3, window='device')
        runs.append((out, list(loop.windowed.batch_rows), list(loop.windowed.idx)))
    (a, rows_a, idx_a), (b, rows_b, _) = runs
    assert a == b and rows_a == rows_b
    assert idx_a == list(range(6))                             # every lead sheet alone is longer than the window
    assert rows_a[0] == 6 and rows_a[-1] < 6 and rows_a == sorted(rows_a, reverse=True)
    for m_before, m_after in zip(rows_a[:-1], rows_a[1:]):     # the rule: a smaller batch is at most half the one before
        assert m_after == m_before or 2 * m_after <= m_before
    assert all(rows_a[t] == rows_a[t - t % 4] for t in range(len(rows_a)))        # row counts change at polls only
    for ids, ld, pr in zip(a, leads, primers):
        _grammar_ok(inf, e2i, i2e, ids, ld, pr)
        assert len(ids) > 48


# ------------------------------------------------------------------------------------------------ the full shape
def _full_vocab():
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4')] + ['Key_%s' % k for k in ('C', 'a', 'G', 'e')] + ['Tempo_110']
             + ['Track_LeadSheet', 'Track_Full', 'Bar_None'] + ['Beat_%d' % i for i in range(16)] + ['Chord_%d_M' % i for i in range(40)])
    names += ['Note_Pitch_%d' % i for i in range(327 - 2 - len(names))] + ['EOS_None', 'PAD_None']
    return {e: i for i, e in enumerate(names)}, dict(enumerate(names))


def _bias_steps(e2i):
    """The output-bias increments of _full_model: bars end after ~15 events, Beats are common, pieces finish."""
    return [(e2i['Track_LeadSheet'], 4.0), (e2i['EOS_None'], 1.0)] + [(e2i['Beat_%d' % k], 2.0) for k in range(16)]


_FULL = {}


def _full_model(kind):
    if kind not in _FULL:
        from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
        from emo_disentanger_amd.model.music_performer import MusicPerformer
        e2i, _ = _full_vocab()
        torch.manual_seed(3)
        if kind == 'performer':
            m = MusicPerformer(327, 12, 8, 512, 2048, 512, favor_feature_dims=128, use_segment_emb=True, n_segment_types=2, compute_dtype='bf16',
                               redraw='fixed')
        else:
            m = MusicGPT2(327, 12, 8, 512, 2048, 512, use_segment_emb=True, n_segment_types=2, dropout=0.1, compute_dtype='bf16')
        with torch.no_grad():
            for w, x in _bias_steps(e2i):
                m.dec_out_proj.bias[w] += x
        _FULL[kind] = m.cuda().eval()
    return _FULL[kind]


FULL_BARS = 150


def _full_batch(e2i, n=8, bars=FULL_BARS):
    rs = np.random.RandomState(1)
    pool = [e2i['Beat_%d' % k] for k in range(16)] + [e2i['Chord_%d_M' % k] for k in range(40)]
    leads = [[[e2i['Bar_None']] + sorted(rs.choice(pool, size=rs.randint(2, 7)).tolist()) for _ in range(bars + i % 2)] for i in range(n)]
    primers = [[e2i['Emotion_Q%d' % (1 + i % 4)], e2i[['Key_C', 'Key_a'][i % 2]], e2i['Tempo_110']] for i in range(n)]
    return leads, primers


def _cpu_piece_lengths(inf, e2i, i2e, leads, primers, temp, top_p, max_events):
    """The host grammar on uniform logits plus the bias of _full_model: what length do these lead sheets give?"""
    logits = np.zeros(len(i2e), np.float32)
    for w, x in _bias_steps(e2i):
        logits[w] += x
    rs = np.random.RandomState(0)
    out = []
    for lead, primer in zip(leads, primers):
        s = inf._Stream(e2i, lead, primer, None)
        while not s.done:
            s.offer(int(inf.nucleus(inf.temperature(logits.copy(), temp), top_p, rng=rs)), e2i, i2e, False, max_events)
        out.append(len(s.result()))
    return out


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_full_shape_pieces_cross_the_window_on_the_device(kind):
    from emo_disentanger_amd import inference as inf
    e2i, i2e = _full_vocab()
    leads, primers = _full_batch(e2i)
    kw = dict(max_events=2600, temp=1.2, top_p=0.9)
    cpu = _cpu_piece_lengths(inf, e2i, i2e, leads, primers, 1.2, 0.9, 2600)
    assert min(cpu) > 2048 + 200, cpu                          # these lead sheets do give pieces well past the window
    assert inf.max_dec_inp_len == 2048
    model = _full_model(kind)
    runs = []
    for _ in range(2):
        loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, seed=4, **kw)
        assert loop.eng.persist is not None                    # the in-window phase runs the one-launch step
        loop.run()
        crossed = [i for i, x in enumerate(loop.state[:, inf.ACC_S_STATUS].cpu().tolist()) if x == inf.ACC_WINDOW]
        out = loop.results(e2i, i2e, 2600, False, 4, window='device')
        runs.append((out, crossed))
    (a, crossed), (b, _) = runs
    assert a == b
    assert len(crossed) >= 6, crossed
    assert loop.windowed.steps >= 100 and loop.windowed.idx == crossed
    for i, (ids, ld, pr) in enumerate(zip(a, leads, primers)):
        _grammar_ok(inf, e2i, i2e, ids, ld, pr)
        if i in crossed:
            assert len(ids) > 2048, (i, len(ids))


# ------------------------------------------------------------------------------------------------ command line
def _cli_setup(tmp_path):
    import yaml
    from oracle.weights import make_state_dict
    g, _, _ = _vocab()
    events = [e for e in g['events'] if e != 'PAD_None']
    e2i = {e: i for i, e in enumerate(events)}
    pickle.dump((e2i, {i: e for e, i in e2i.items()}), open(tmp_path / 'dictionary_functional.pkl', 'wb'))
    V = len(events) + 1
    sd = make_state_dict('gpt2', V, 2, 4, 64, 128, seed=3, scale=2.0)
    sd['dec_out_proj.bias'][e2i['Track_LeadSheet']] += 3.0     # bars end soon
    sd['dec_out_proj.bias'][V - 1] -= 30.0                     # the pad id has no event name
    torch.save(sd, tmp_path / 'params.pt')
    conf = {'training': {'gpuid': 0}, 'data_loader': {'vocab_path': str(tmp_path / 'dictionary_{}.pkl')},
            'model': {'n_layer': 2, 'n_head': 4, 'd_model': 64, 'd_ff': 128, 'd_embed': 64, 'use_segemb': True, 'feature_map': {'n_dims': 32}}}
    yaml.safe_dump(conf, open(tmp_path / 'conf.yaml', 'w'))
    out = tmp_path / 'gen'
    out.mkdir()
    bars = ['Bar_None', 'Beat_0', 'Chord_I_M', 'Beat_8', 'Chord_V_M']
    sheets = {'samp_00_Positive_roman.txt': ['Key_C'] + bars * 14, 'samp_01_Q3_roman.txt': ['Key_a'] + bars * 2}
    for f, lines in sheets.items():                            # as the stage-1 command line writes them
        (out / f).write_text('\n'.join(lines) + '\n')
    return e2i, out, ['-m', 'gpt2', '-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '-i', str(tmp_path / 'params.pt'), '-o', str(out),
                      '--streams', '3', '--dtype', 'fp32', '--max_bars', '16']


def test_command_line_window_device_writes_pieces_past_the_window(tmp_path, monkeypatch):
    from emo_disentanger_amd import inference as inf
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    e2i, out, argv = _cli_setup(tmp_path)
    inf.main(argv + ['--device', '--window', 'device'])
    written = sorted(f for f in os.listdir(out) if f.endswith('_full.txt'))
    assert written == ['samp_00_Q1_full.txt', 'samp_00_Q4_full.txt', 'samp_01_Q3_full.txt']
    for f in written:
        lines = (out / f).read_text().splitlines()
        src = out / ('samp_00_Positive_roman.txt' if f.startswith('samp_00') else 'samp_01_Q3_roman.txt')
        key, bars = inf.read_lead_sheet(str(src), e2i)
        assert all(x in e2i for x in lines) and lines[0] == key
        ids = [e2i[x] for x in lines[1:]]
        if f.startswith('samp_00'):                            # 14 bars of 5 events and their Track_* marks alone pass the 48-token window
            assert len(ids) > 14 * 7 > 48
        for b in bars:                                         # every injected lead-sheet bar is in the piece, followed by Track_Full
            run = [e2i['Track_LeadSheet']] + b + [e2i['Track_Full']]
            assert any(ids[j:j + len(run)] == run for j in range(len(ids))), (f, b)
        assert ids.count(e2i['Track_LeadSheet']) == len(bars)


def test_command_line_window_device_needs_device(tmp_path, capsys):
    from emo_disentanger_amd import inference as inf
    _, out, argv = _cli_setup(tmp_path)
    with pytest.raises(SystemExit) as e:
        inf.main(argv + ['--window', 'device'])
    assert e.value.code == 2 and '--window device needs --device' in capsys.readouterr().err
    assert not [f for f in os.listdir(out) if f.endswith('_full.txt')]
