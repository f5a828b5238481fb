"""GPU: stage-2 accompaniments on the device — the grammar step emo_acc_grammar_step against a host restatement on _Stream, the graph-replayed
device loop generate_accompaniments against the host grammar driven by the same device draws (tiny models on the launch chain, the full
shape on the one-launch persistent step), the window handoff and the --device command line."""
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


def _tiny(kind, dtype):
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    from oracle.weights import make_state_dict
    m = json.load(open(os.path.join(G, 'generate.json')))['model']
    if kind == 'gpt2':
        sd = make_state_dict('gpt2', m['V'], m['L'], m['H'], m['d'], m['dff'], seed=m['seed'], scale=m['scale'])
        mod = MusicGPT2(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], dropout=0.1, use_segment_emb=True, n_segment_types=2, compute_dtype=dtype)
    else:
        sd = make_state_dict('performer', m['V'], m['L'], m['H'], m['d'], m['dff'], favor_feature_dims=32, seed=m['seed'], scale=m['scale'])
        mod = MusicPerformer(m['V'], m['L'], m['H'], m['d'], m['dff'], m['d'], favor_feature_dims=32, use_segment_emb=True, n_segment_types=2,
                             compute_dtype=dtype, redraw='fixed')
    mod.load_state_dict(sd)
    return mod.cuda().eval()


# ------------------------------------------------------------------------------------------------ the kernel, launch by launch
class HostAcc:
    """Host restatement of one stream of emo_acc_grammar_step on _Stream.offer (the grammar of generate_conditional)."""

    def __init__(self, inf, e2i, i2e, lead, primer, max_bars, max_events, skip_check, L0, W):
        self.inf, self.e2i, self.i2e = inf, e2i, i2e
        self.s = inf._Stream(e2i, lead, primer, max_bars)
        self.s.consumed = L0
        self.max_events, self.skip, self.W = max_events, skip_check, W
        self.status = inf.ACC_DONE if self.s.done else inf.ACC_RUNNING
        self.draws = self.accepted = 0
        self.tok = self.seg = None

    def wants_draw(self):
        s = self.s
        return self.status == self.inf.ACC_RUNNING and len(s.generated) < self.W and s.consumed == len(s.generated)

    def step(self, pick, n_u):
        """pick(d) -> the word the d-th draw of this stream gives."""
        inf, s = self.inf, self.s
        pad = self.e2i['PAD_None']
        if self.status != inf.ACC_RUNNING:
            self.tok, self.seg = pad, 1
            return
        if len(s.generated) >= self.W:
            self.status, self.tok, self.seg = inf.ACC_WINDOW, pad, 1
            return
        if s.consumed == len(s.generated):
            while True:
                if self.draws >= n_u:
                    self.status = inf.ACC_OUT_OF_DRAWS
                    break
                w = pick(self.draws)
                self.draws += 1
                ok = s.offer(w, self.e2i, self.i2e, self.skip, self.max_events)
                if s.stuck:
                    self.status = inf.ACC_STUCK
                    break
                if ok:
                    self.accepted += 1
                    if s.done:
                        self.status = inf.ACC_DONE
                    break
        if self.status == inf.ACC_RUNNING:
            self.tok, self.seg = s.generated[s.consumed], s.seg[s.consumed]
            s.consumed += 1
        else:
            self.tok, self.seg = pad, 1

    def state(self):
        inf, s = self.inf, self.s
        d = {inf.ACC_S_STATUS: self.status, inf.ACC_S_LEN: len(s.generated), inf.ACC_S_BARS: s.generated_bars, inf.ACC_S_CUR_POS: s.cur_pos,
             inf.ACC_S_FAILED: s.failed_cnt, inf.ACC_S_DRAWS: self.draws, inf.ACC_S_ACCEPTED: self.accepted}
        if self.status == inf.ACC_RUNNING:
            d[inf.ACC_S_CONSUMED] = s.consumed
        return d


B = lambda k: 'Beat_%d' % k      # noqa: E731
# per stream: lead sheet (bar indices into generate.json's lead), primer, max_bars, max_events, skip_check, u overrides {draw: u},
# and per launch that draws: the candidate words (one-hot: that word; two: the lower id for u < 0.5, the higher for u >= 0.5)
UNIT = [
    # Beat going backwards: rejected, then a redraw in the SAME launch; Track_LeadSheet mid-piece (bar injection, cur_pos reset), then at the
    # last bar -> DONE
    ([0, 1], [0, 4, 6], None, 200, False, {1: 0.2, 2: 0.8}, [[B(5)], [B(2), B(8)], ['Note_Octave_4'], ['Track_LeadSheet'], [B(0)], ['Track_LeadSheet']]),
    # 256 Beats in a row below the position -> STUCK inside one launch
    ([0, 1, 2], [1, 5, 6], None, 200, False, {}, [[B(6)], [B(1)]]),
    # PAD and a premature EOS (rejected, not counted), then EOS at the last bar -> DONE
    ([0, 2], [0, 4, 6], None, 200, False, {0: 0.8, 1: 0.2, 2: 0.8, 3: 0.2},
     [['Chord_I_M', 'PAD_None'], ['Note_Degree_1', 'EOS_None'], ['Track_LeadSheet'], [B(3)], ['EOS_None']]),
    # max_events
    ([0, 1, 2], [2, 4, 6], None, 14, False, {}, [['Note_Octave_4'], [B(1)], ['Note_Degree_1'], ['Chord_V_M']]),
    # skip_check: a Beat below the position is accepted; max_bars = 1: the first Track_LeadSheet ends the piece
    ([1, 0], [3, 5, 6], 1, 200, True, {}, [[B(7)], [B(2)], [B(0)], ['Track_LeadSheet']]),
    # a primer longer than L0 (fed token by token, no draws), a Beat rejected and a Track_LeadSheet accepted in one launch
    ([2, 0], [0, 4, 6, 26, 27, 28, 29], None, 200, False, {1: 0.8, 2: 0.2}, [[B(9)], [B(4), 'Track_LeadSheet'], ['Track_LeadSheet']]),
    # PAD forever: the uniform table runs out -> OUT_OF_DRAWS
    ([0], [1, 4, 6], None, 200, False, {}, [['Note_Octave_4'], ['PAD_None']]),
    # the row reaches the window (max_len = W below) -> WINDOW
    ([0, 1, 2], [2, 5, 6], None, 200, False, {}, [['Note_Velocity_60']] * 40),
]
W_UNIT, NU_UNIT = 40, 300


def test_grammar_kernel_matches_the_host_grammar_step_by_step():
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    V, n, dev = len(i2e), len(UNIT), 'cuda'
    leads = [[list(g['lead'][j]) for j in u[0]] for u in UNIT]
    L0 = min(len(u[1]) + 2 + len(ld[0]) for u, ld in zip(UNIT, leads))
    hosts = [HostAcc(inf, e2i, i2e, ld, u[1], u[2], u[3], u[4], L0, W_UNIT) for u, ld in zip(UNIT, leads)]
    scripts = [[[e2i[w] for w in c] for c in u[6]] for u in UNIT]
    U = np.full((NU_UNIT, n), 0.2, np.float32)
    for i, u in enumerate(UNIT):
        for d, val in u[5].items():
            U[d, i] = val
    flags, beat = inf.acc_event_tables(i2e, V)
    toks, offs, bar0, nbars, longest = inf.pack_lead_sheets(leads)
    width = W_UNIT + longest + 2
    seq, segs = np.zeros((n, width), np.int64), np.zeros((n, width), np.int64)
    params, state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
    for i, (h, u) in enumerate(zip(hosts, UNIT)):
        k = len(h.s.generated)
        seq[i, :k], segs[i, :k] = h.s.generated, h.s.seg
        params[i, :5] = h.s.target_bars, u[3], u[4], bar0[i], nbars[i]
        state[i, [inf.ACC_S_STATUS, inf.ACC_S_LEN, inf.ACC_S_CONSUMED]] = h.status, k, L0
    T = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    seq_d, segs_d, params_d, state_d, U_d = T(seq), T(segs), T(params), T(state), T(U)
    ev_flags, ev_beat, lead_tok, lead_off = T(flags), T(beat), T(toks), T(offs)
    running = torch.tensor([sum(h.status == inf.ACC_RUNNING for h in hosts)], dtype=torch.int32, device=dev)
    tok = torch.full((n,), -1, dtype=torch.long, device=dev)
    seg = torch.full((n,), -1, dtype=torch.long, device=dev)
    launches = [0] * n
    steps = 0
    while any(h.status == inf.ACC_RUNNING for h in hosts):
        logits = np.zeros((n, V), np.float32)
        cands = [None] * n
        for i, h in enumerate(hosts):
            if h.wants_draw():
                cands[i] = sorted(scripts[i][launches[i]])
                launches[i] += 1
                logits[i, cands[i]] = 60.0              # one or two equally likely words: the nucleus keeps exactly those
        ops.acc_grammar_step(T(logits), 1.2, 0.9, U_d, ev_flags, ev_beat, lead_tok, lead_off, params_d, state_d, seq_d, segs_d, W_UNIT,
                             e2i['Track_Full'], e2i['PAD_None'], tok, seg, running)
        for i, h in enumerate(hosts):
            c = cands[i]
            h.step(lambda d, c=c, i=i: c[0] if U[d, i] < 0.5 else c[-1], NU_UNIT)
        st, sq, sg, tk, sk = (x.cpu().numpy() for x in (state_d, seq_d, segs_d, tok, seg))
        for i, h in enumerate(hosts):
            for k, v in h.state().items():
                assert st[i, k] == v, (steps, i, k, st[i].tolist())
            assert sq[i, :len(h.s.generated)].tolist() == h.s.generated, (steps, i)
            assert sg[i, :len(h.s.seg)].tolist() == h.s.seg, (steps, i)
            assert (tk[i], sk[i]) == (h.tok, h.seg), (steps, i)
        assert int(running.item()) == sum(h.status == inf.ACC_RUNNING for h in hosts)
        steps += 1
        assert steps < 200
    want = [inf.ACC_DONE, inf.ACC_STUCK, inf.ACC_DONE, inf.ACC_DONE, inf.ACC_DONE, inf.ACC_DONE, inf.ACC_OUT_OF_DRAWS, inf.ACC_WINDOW]
    assert [h.status for h in hosts] == want
    assert launches[:7] == [len(s) for s in scripts[:7]]                    # every scripted launch was used, nothing more
    assert hosts[0].draws == 7 and hosts[1].draws == 257 and hosts[6].draws == NU_UNIT
    assert hosts[0].s.generated_bars == 2 and hosts[4].s.generated_bars == 1
    assert len(hosts[3].s.generated) == 15 and len(hosts[7].s.generated) == W_UNIT


def _three_streams(inf, g, e2i, i2e, dev, n_u=8):
    """Three streams of UNIT on the device, for the argument-block tests: 0 finished before the first launch, 1 still feeding a primer two tokens
    longer than the common prefix, 2 drawing from the first launch; a uniform table of n_u rows.  -> (what the launches only read, a maker of
    fresh copies of what they write), both keyed by the fields of emo_grammar_step_t."""
    pick = [UNIT[0], UNIT[5], UNIT[6]]
    V, n = len(i2e), len(pick)
    leads = [[list(g['lead'][j]) for j in u[0]] for u in pick]
    st = [inf._Stream(e2i, ld, u[1], u[2]) for u, ld in zip(pick, leads)]
    L0 = min(len(s.generated) for s in st)
    flags, beat = inf.acc_event_tables(i2e, V)
    toks, offs, bar0, nbars, longest = inf.pack_lead_sheets(leads)
    width = W_UNIT + longest + 2
    seq, segs = np.zeros((n, width), np.int64), np.zeros((n, width), np.int64)
    params, state = np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
    for i, (s, u) in enumerate(zip(st, pick)):
        k = len(s.generated)
        seq[i, :k], segs[i, :k] = s.generated, s.seg
        params[i, :5] = s.target_bars, u[3], u[4], bar0[i], nbars[i]
        state[i, [inf.ACC_S_STATUS, inf.ACC_S_LEN, inf.ACC_S_CONSUMED]] = inf.ACC_RUNNING, k, L0
    state[0, inf.ACC_S_STATUS] = inf.ACC_DONE
    T = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    shared = dict(u_steps=torch.rand(n_u, n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)), ev_flags=T(flags), ev_beat=T(beat),
                  lead_tok=T(toks), lead_off=T(offs), params=T(params))
    fresh = lambda: dict(state=T(state), seq=T(seq), segs=T(segs), tok_out=torch.full((n,), -1, dtype=torch.long, device=dev),      # noqa: E731
                         seg_out=torch.full((n,), -1, dtype=torch.long, device=dev), running=torch.tensor([2], dtype=torch.int32, device=dev))
    return shared, fresh


def test_a_prepared_grammar_block_reused_over_steps_equals_the_one_shot_wrapper():
    # stream 2 accepts one word, then draws PAD until its table of 8 uniforms is used up (OUT_OF_DRAWS inside the second launch); stream 1 feeds
    # two primer tokens, then draws from random logits.  A GrammarStep filled once and launched six times leaves, word for word, what
    # ops.acc_grammar_step (a fresh block per call) leaves on its own copies of the same tensors.
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    V, n, dev = len(i2e), 3, 'cuda'
    shared, fresh = _three_streams(inf, g, e2i, i2e, dev)
    one, blk = fresh(), fresh()
    logits = torch.randn(6, n, V, device=dev, generator=torch.Generator(device=dev).manual_seed(6)) * 2.0
    logits[0, 2, e2i['Note_Octave_4']] = 60.0
    logits[1:, 2, e2i['PAD_None']] = 60.0
    lg = torch.empty(n, V, device=dev)
    tf, pad = e2i['Track_Full'], e2i['PAD_None']
    args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
    ops.block_set(args, held, n_rows=n, n_token=V, ld_u=n, temperature=1.2, top_p=0.9, max_len=W_UNIT, track_full=tf, pad=pad, logits=lg, **shared, **blk)
    for t in range(6):
        lg.copy_(logits[t])
        ops.acc_grammar_step(lg, 1.2, 0.9, shared['u_steps'], shared['ev_flags'], shared['ev_beat'], shared['lead_tok'], shared['lead_off'],
                             shared['params'], one['state'], one['seq'], one['segs'], W_UNIT, tf, pad, one['tok_out'], one['seg_out'], one['running'])
        ops.grammar_step(args)
        for k in one:
            assert torch.equal(one[k], blk[k]), (t, k, one[k].tolist(), blk[k].tolist())
    st = blk['state'].cpu().numpy()
    assert st[0, inf.ACC_S_STATUS] == inf.ACC_DONE and st[2, inf.ACC_S_STATUS] == inf.ACC_OUT_OF_DRAWS and st[2, inf.ACC_S_DRAWS] == 8
    assert st[2, inf.ACC_S_ACCEPTED] == 1 and st[1, inf.ACC_S_DRAWS] >= 1 and st[0, inf.ACC_S_DRAWS] == 0
    assert blk['tok_out'].cpu().tolist()[0::2] == [pad, pad] and blk['seg_out'].cpu().tolist()[0::2] == [1, 1]


def test_the_block_setter_refuses_a_bad_layout_when_the_tensor_enters_the_block():
    # the asserts of the former per-call wrappers, now made once: a tensor of the wrong shape, stride or dtype never gets its address into a
    # GrammarStep (no launch is made here)
    from emo_disentanger_amd import inference as inf, ops
    g, e2i, i2e = _vocab()
    V, n, dev = len(i2e), 3, 'cuda'
    shared, fresh = _three_streams(inf, g, e2i, i2e, dev)
    good = dict(shared, logits=torch.zeros(n, V, device=dev), **fresh())
    numbers = dict(n_rows=n, n_token=V, ld_u=n, temperature=1.2, top_p=0.9, max_len=W_UNIT, track_full=e2i['Track_Full'], pad=e2i['PAD_None'])
    wide = torch.zeros(n, 2 * good['seq'].shape[1], dtype=torch.int64, device=dev)
    for field, bad in (('state', good['state'][:, :7].contiguous()), ('seq', wide[:, ::2]), ('ev_flags', good['ev_flags'].long()),
                       ('u_steps', torch.zeros(8, n + 1, device=dev))):
        args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
        with pytest.raises(AssertionError, match='grammar step: bad dtype / layout of %s' % field):
            ops.block_set(args, held, **numbers, **dict(good, **{field: bad}))
        assert field not in held and getattr(args, field) is None                  # (a c_void_p field reads as None while it is NULL)
    args, held = ops.GrammarStep(kind=ops.GRAMMAR_ACC), {}
    ops.block_set(args, held, **numbers, **good)
    assert args.state == good['state'].data_ptr() and args.ld_seq == good['seq'].shape[1] and args.n_u == 8 and held['segs'] is good['segs']


# ------------------------------------------------------------------------------------------------ the device loop against the host grammar
def _host_grammar_loop(inf, model, e2i, i2e, leads, primers, U, max_events, skip_check, temp, top_p, max_bars=None):
    """The same engine, ops.sample_nucleus on each stream's own column of U at its own draw counter, _Stream.offer on the host."""
    from emo_disentanger_amd import ops
    n, W = len(leads), inf.max_dec_inp_len
    dev = U.device
    st = [inf._Stream(e2i, leads[i], primers[i], max_bars) for i in range(n)]
    status = [inf.ACC_DONE if s.done else inf.ACC_RUNNING for s in st]
    draws = [0] * n
    pad = e2i['PAD_None']
    with torch.no_grad():
        eng = inf.make_engine(model, n, redraw=False) if model.kind == 'performer' else inf.GPT2DecodeEngine(model, n, max_len=W)
        L0 = min(len(s.generated) for s in st)
        logits = eng.prefill(torch.tensor([s.generated[:L0] for s in st], device=dev), torch.tensor([s.seg[:L0] for s in st], device=dev))
        for s in st:
            s.consumed = L0
        while True:
            want = [i for i in range(n) if status[i] == inf.ACC_RUNNING and len(st[i].generated) < W and st[i].consumed == len(st[i].generated)]
            for i in range(n):
                if status[i] == inf.ACC_RUNNING and len(st[i].generated) >= W:
                    status[i] = inf.ACC_WINDOW
            while want:                                     # one draw for every stream that wants one, again for the rejected ones
                ctr = torch.tensor([min(d, U.shape[0] - 1) for d in draws], device=dev)
                u = U.gather(0, ctr.view(1, n)).view(n).contiguous()
                words = ops.sample_nucleus(logits.contiguous(), temp, top_p, u).cpu().tolist()
                again = []
                for i in want:
                    if draws[i] >= U.shape[0]:
                        status[i] = inf.ACC_OUT_OF_DRAWS
                        continue
                    draws[i] += 1
                    ok = st[i].offer(words[i], e2i, i2e, skip_check, max_events)
                    if st[i].stuck:
                        status[i] = inf.ACC_STUCK
                    elif ok:
                        status[i] = inf.ACC_DONE if st[i].done else status[i]
                    else:
                        again.append(i)
                want = again
            if all(x != inf.ACC_RUNNING for x in status):
                break
            tok, seg = [pad] * n, [1] * n
            for i, s in enumerate(st):
                if status[i] == inf.ACC_RUNNING:
                    tok[i], seg[i] = s.generated[s.consumed], s.seg[s.consumed]
                    s.consumed += 1
            logits = eng.step(torch.tensor(tok, device=dev), torch.tensor(seg, device=dev)).clone()
    return st, status


def _expected(inf, st, status):
    return [s.generated[:-1] if x == inf.ACC_DONE else s.generated if x == inf.ACC_STUCK else None for s, x in zip(st, status)]


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('skip_check', [False, True])
def test_device_loop_equals_host_grammar_on_the_same_draws(kind, dtype, skip_check):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    model = _tiny(kind, dtype)
    lead = [list(b) for b in g['lead']]
    leads = [lead, lead[::-1], lead[:2], [lead[1]] * 4, lead + lead, [lead[2]]]
    primers = [list(g['primer']), [1, 5, 6], list(g['primer']), [2, 4], [3, 5, 6], [0, 4, 6, 26, 27]]
    kw = dict(max_events=150, skip_check=skip_check, temp=1.2, top_p=0.97, seed=5)
    got, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, use_graph=True, **kw)
    eager, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, use_graph=False, **kw)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)           # (the loop's uniform table, unused otherwise)
    st, status = _host_grammar_loop(inf, model, e2i, i2e, leads, primers, loop.U, 150, skip_check, 1.2, 0.97)
    assert got == _expected(inf, st, status)
    assert eager == got
    assert len({tuple(r) for r in got}) == len(leads)


# ------------------------------------------------------------------------------------------------ the full shape (one-launch persistent step)
def _full_vocab():
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4')] + ['Key_%s' % k for k in ('C', 'a', 'G', 'e')] + ['Tempo_110']
             + ['Track_LeadSheet', 'Track_Full', 'Bar_None'] + ['Beat_%d' % i for i in range(16)] + ['Chord_%d_M' % i for i in range(40)])
    names += ['Note_Pitch_%d' % i for i in range(327 - 2 - len(names))] + ['EOS_None', 'PAD_None']
    return {e: i for i, e in enumerate(names)}, dict(enumerate(names))


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
        with torch.no_grad():                      # bars end after ~15 events, Beats are common, pieces finish
            b = m.dec_out_proj.bias
            b[e2i['Track_LeadSheet']] += 4.0
            b[e2i['EOS_None']] += 1.0
            for k in range(16):
                b[e2i['Beat_%d' % k]] += 2.0
        _FULL[kind] = m.cuda().eval()
    return _FULL[kind]


def _full_batch(e2i, n=32, bars=3):
    rs = np.random.RandomState(1)
    pool = [e2i['Beat_%d' % k] for k in range(16)] + [e2i['Chord_%d_M' % k] for k in range(40)]
    leads = [[[e2i['Bar_None']] + sorted(rs.choice(pool, size=rs.randint(2, 7)).tolist()) for _ in range(bars + i % 2)] for i in range(n)]
    primers = [[e2i['Emotion_Q%d' % (1 + i % 4)], e2i[['Key_C', 'Key_a'][i % 2]], e2i['Tempo_110']] for i in range(n)]
    return leads, primers


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_full_shape_device_loop_on_the_persistent_step_equals_host_grammar(kind):
    from emo_disentanger_amd import inference as inf
    e2i, i2e = _full_vocab()
    model = _full_model(kind)
    leads, primers = _full_batch(e2i)
    kw = dict(max_events=10000, skip_check=False, temp=1.2, top_p=0.9, seed=11)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
    assert loop.eng.persist is not None                      # the one-launch step runs this shape
    loop.run(use_graph=True)
    got = loop.results(e2i, i2e, 10000, False, 11)
    st, status = _host_grammar_loop(inf, model, e2i, i2e, leads, primers, loop.U, 10000, False, 1.2, 0.9)
    assert got == _expected(inf, st, status)
    assert loop.counts()['finished'] >= 24


@pytest.mark.parametrize('kind', ['performer', 'gpt2'])
def test_full_shape_pieces_obey_the_grammar(kind):
    from emo_disentanger_amd import inference as inf
    e2i, i2e = _full_vocab()
    model = _full_model(kind)
    leads, primers = _full_batch(e2i)
    kw = dict(max_events=10000, temp=1.2, top_p=0.9, seed=4)
    a, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **kw)
    b, _ = inf.generate_accompaniments(model, e2i, i2e, leads, primers, **kw)
    assert a == b
    tls, tf = e2i['Track_LeadSheet'], e2i['Track_Full']
    finished = 0
    for ids, lead, primer in zip(a, leads, primers):
        assert isinstance(ids, list), ids
        assert ids[:len(primer)] == primer and e2i['PAD_None'] not in ids
        starts = [j for j, w in enumerate(ids) if w == tls]
        if len(starts) != len(lead):                          # stuck (256 Beats going back): it ends mid-bar
            continue
        finished += 1
        for k, j in enumerate(starts):                        # every Track_LeadSheet is followed by the input bar and Track_Full
            assert ids[j + 1:j + 2 + len(lead[k])] == lead[k] + [tf], k
            body = ids[j + 2 + len(lead[k]):(starts[k + 1] if k + 1 < len(starts) else len(ids))]
            beats = [inf.beat_position(i2e[w]) for w in body if 'Beat' in i2e[w]]
            assert beats == sorted(beats), (k, beats)
    assert finished >= 24


# ------------------------------------------------------------------------------------------------ window handoff, command line
def test_window_handoff_continues_the_device_prefix(monkeypatch):
    from emo_disentanger_amd import inference as inf
    g, e2i, i2e = _vocab()
    monkeypatch.setattr(inf, 'max_dec_inp_len', 48)
    model = _tiny('gpt2', 'fp32')
    lead = [list(b) for b in g['lead']]
    leads, primers = [lead * 4, lead, lead * 3], [list(g['primer']), [1, 5, 6], [2, 4, 6]]
    kw = dict(max_events=400, skip_check=False, temp=1.2, top_p=0.97, seed=9)
    loop = inf.AccompanimentLoop(model, e2i, i2e, leads, primers, **kw)
    loop.run()
    assert loop.eng.max_len == 48 and loop.pos <= 48
    status = loop.state[:, inf.ACC_S_STATUS].cpu().tolist()
    got = loop.results(e2i, i2e, 400, False, 9)
    st, ref_status = _host_grammar_loop(inf, model, e2i, i2e, leads, primers, loop.U, 400, False, 1.2, 0.97)
    assert status == ref_status and inf.ACC_WINDOW in status
    for i, (s, x) in enumerate(zip(st, ref_status)):
        if x != inf.ACC_WINDOW:
            assert got[i] == _expected(inf, [s], [x])[0]
            continue
        assert len(s.generated) >= 48 and got[i][:len(s.generated)] == s.generated       # the device prefix, up to the handoff
        rs = np.random.RandomState([9, i])
        rest = inf._resume_windowed(model, e2i, i2e, s, 400, False, 1.2, None, lambda p, rs=rs: inf.nucleus(p, 0.97, rng=rs))
        assert got[i] == rest and len(rest) >= 48


def test_command_line_device_writes_accompaniments(tmp_path):
    import yaml
    from emo_disentanger_amd import inference as inf
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
    sheets = {'samp_00_Positive_roman.txt': ['Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M', 'Bar_None', 'Beat_4', 'Chord_V_M'],
              'samp_01_Negative_roman.txt': ['Key_a', 'Bar_None', 'Beat_0', 'Chord_V_M', 'Bar_None', 'Beat_0', 'Chord_I_M', 'Bar_None', 'Beat_8']}
    for f, lines in sheets.items():                            # as the stage-1 command line writes them
        (out / f).write_text('\n'.join(lines) + '\n')
    inf.main(['-m', 'gpt2', '-c', str(tmp_path / 'conf.yaml'), '-r', 'functional', '-i', str(tmp_path / 'params.pt'), '-o', str(out),
              '--streams', '3', '--dtype', 'fp32', '--max_bars', '8', '--device'])
    written = sorted(f for f in os.listdir(out) if f.endswith('_full.txt'))
    assert written == ['samp_00_Q1_full.txt', 'samp_00_Q4_full.txt', 'samp_01_Q2_full.txt', 'samp_01_Q3_full.txt']
    for f in written:
        lines = (out / f).read_text().splitlines()
        src = out / ('samp_0%s_%s_roman.txt' % (f[6], 'Positive' if f[8:10] in ('Q1', 'Q4') else 'Negative'))
        key, bars = inf.read_lead_sheet(str(src), e2i)
        assert all(x in e2i for x in lines)
        assert lines[0] == key and lines[1] == 'Emotion_' + f[8:10] and lines[2] == key
        ids = [e2i[x] for x in lines[1:]]
        for b in bars:                                         # every injected lead-sheet bar is in the piece, followed by Track_Full
            run = [e2i['Track_LeadSheet']] + b + [e2i['Track_Full']]
            assert any(ids[j:j + len(run)] == run for j in range(len(ids))), (f, b)
