"""GPU: the stage-1 Transformer-XL token step as one persistent launch (emo_decode_step form 2, pd_step_kernel<2> of csrc/emo_decode_persist.hip)
against (a) the chain of launches it replaces (PlainTransformer.decode_step: the same bf16 arithmetic up to the reduction order — logits within
2 % of the logit range, appended key / value rows within 1e-2 relative norm), (b) the fp32 model's chain (5 %), (c) the oracle fed one token at a
time with its mems (5 %), and through generate_lead_sheets(step='one_launch'): host grammar on the same device draws, graph replay = eager
launches, the cache's last row, and the refusals.  Bounds: those of the GPT-2 form in tests/test_gpu_decode_persistent.py.
Reference: stage1_compose/model/plain_transformer.py:52-59 (generate), optimus_txl_decoder.py:301-391, 526-557; loop inference_utils.py:51-134."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, H, D, DFF = 200, 8, 512, 2048          # V is no multiple of the 16-column logits tile


def _sd(L, seed=3, scale=2.0):
    from oracle.txl_ref import make_state_dict_txl
    return make_state_dict_txl(V, L, H, D, DFF, seed=seed, scale=scale)


def _model(L, mem_len, dtype='bf16', sd=None, max_gen_len=1024, d=D, pre_lnorm=True):
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    m = PlainTransformer(d, V, L, H, d, DFF, mem_len, mem_len, dec_dropout=0.1, pre_lnorm=pre_lnorm, compute_dtype=dtype, max_gen_len=max_gen_len)
    if sd is not None:
        m.load_state_dict(sd)
    return m.cuda().eval()


def _teacher_force(m, ptok, toks, one_launch):
    """-> (logits [n, K + 1, V] fp32: the prefill's and each step's, K caches, V caches as [n, H, T, dh] of the first T0 + K rows)."""
    from emo_disentanger_amd import stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import TXLMemory, head_major
    n, T0 = ptok.shape
    K = toks.shape[1]
    with torch.no_grad():
        mem = TXLMemory(m, n, m._max_gen_len)
        h, _, _ = m._prefill(ptok.t(), mem)
        out = [m._logits(h.view(n, T0, -1)[:, -1].contiguous()).float().clone()]
        if one_launch:
            st = s1.OneLaunchStep(m, n, r_dist=mem.r_dist).take_over(mem, T0)
            for t in range(K):
                out.append(st.step(toks[:, t]).float().clone())
            st.check_persistent()
            assert int(st.mem.lens.min()) == T0 + K == int(st.mem.lens.max())
            kc, vc = [k[:, :, :T0 + K].clone() for k in st.mem.kc], [v[:, :, :T0 + K].clone() for v in st.mem.vc]
        else:
            for t in range(K):
                out.append(m.decode_step(toks[:, t], mem).float().clone())
            kc = [head_major(k[:, :T0 + K], H).clone() for k in mem.kc]
            vc = [head_major(v[:, :T0 + K], H).clone() for v in mem.vc]
    return torch.stack(out, 1), kc, vc


@pytest.mark.parametrize('n,L,T0,mem_len,K', [(4, 1, 3, 8, 14),        # the window starts to slide in the middle of the run
                                              (5, 2, 1, 8, 12),        # a padded second group, a one-token primer
                                              (1, 2, 600, 512, 6),     # a prefill longer than the window: j0 > 0 from the first step
                                              (32, 12, 40, 512, 6)])   # the product shape
def test_one_launch_step_matches_the_chain_and_fp32(n, L, T0, mem_len, K):
    g = torch.Generator().manual_seed(21 + n)
    ptok = torch.randint(0, V - 1, (n, T0), generator=g).cuda()
    toks = torch.randint(0, V - 1, (n, K), generator=g).cuda()
    sd = _sd(L)
    mb = _model(L, mem_len, 'bf16', sd)
    one, K1, V1 = _teacher_force(mb, ptok, toks, True)              # (check_persistent inside, before any assertion)
    chain, K0, V0 = _teacher_force(mb, ptok, toks, False)
    ref, _, _ = _teacher_force(_model(L, mem_len, 'fp32', sd), ptok, toks, False)
    rng = float(ref.max() - ref.min())
    e_chain = float((one - chain).abs().max()) / rng
    e_ref = float((one - ref).abs().max()) / rng
    e_chain_ref = float((chain - ref).abs().max()) / rng
    e_kv = max(float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)) for a, b in zip(K1 + V1, K0 + V0))
    print('[one-launch TXL step] n=%d L=%d T0=%d mem_len=%d: vs chain %.4f, vs fp32 %.4f (chain vs fp32 %.4f) of the logit range; K / V rows %.2e'
          % (n, L, T0, mem_len, e_chain, e_ref, e_chain_ref, e_kv))
    assert torch.equal(one[:, 0], chain[:, 0])                       # the prefill is shared
    assert e_chain <= 0.02 and e_ref <= 0.05
    for a, b in zip(K1 + V1, K0 + V0):
        assert a.shape == b.shape and float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-12)) <= 1e-2


def test_one_launch_step_matches_the_oracle_fed_one_token_at_a_time():
    from oracle import txl_ref
    n, L, T0, mem_len, K = 4, 2, 4, 8, 20
    g = torch.Generator().manual_seed(77)
    tok = torch.randint(0, V - 1, (n, T0 + K), generator=g)
    sd = _sd(L)
    with torch.no_grad():
        lg, mems = txl_ref.forward(sd, tok[:, :T0].t(), L, H, mems=None, mem_len=mem_len)
        ref = [lg[-1]]
        for t in range(K):
            lg, mems = txl_ref.forward(sd, tok[:, T0 + t:T0 + t + 1].t(), L, H, mems=mems, mem_len=mem_len)
            ref.append(lg[-1])
    ref = torch.stack(ref, 1)                                        # [n, K + 1, V]
    tc = tok.cuda()
    got, _, _ = _teacher_force(_model(L, mem_len, 'bf16', sd), tc[:, :T0], tc[:, T0:], True)
    rng = float(ref.max() - ref.min())
    err = (got.cpu() - ref).abs().amax(dim=(0, 2))
    print('[one-launch TXL step vs oracle] max |dlogit| %.4f of the logit range (prefill %.4f, step 1 %.4f, step %d %.4f)'
          % (float(err.max()) / rng, float(err[0]) / rng, float(err[1]) / rng, K, float(err[-1]) / rng))
    assert float(err.max()) <= 0.05 * rng


# ------------------------------------------------------------------------------------------------ the loop
def _toy_vocab():
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative')]
             + ['Key_%s' % k for k in ('C', 'C#', 'D', 'D#', 'E', 'F', 'F#', 'G', 'G#', 'A', 'A#', 'B')]
             + ['Key_%s' % k for k in ('c', 'c#', 'd', 'd#', 'e', 'f', 'f#', 'g', 'g#', 'a', 'a#', 'b')]
             + ['Bar_None'] + ['Beat_%d' % i for i in range(16)] + ['Tempo_%d' % t for t in range(60, 180, 10)])
    names += ['Chord_%d_%d' % (i // 8, i % 8) for i in range(88)]
    names += ['Note_Degree_%d' % i for i in range(V - 2 - len(names))] + ['EOS_None', 'PAD_None']
    assert len(names) == V
    return {e: i for i, e in enumerate(names)}, dict(enumerate(names))


STREAMS6 = [  # primer, representation, key_determine, max_bars, max_events, prompt_bars  (6 streams: a padded second group)
    (['Emotion_Q1'], 'functional', None, 3, 40, None), (['Emotion_Q2'], 'functional', 'rule', 4, 36, None),
    (['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_0_1'], 'functional', None, 3, 44, 1),
    (None, 'remi', None, 2, 30, None), (['Emotion_Negative'], 'functional', 'rule', 3, 40, None), (['Emotion_Q2'], 'functional', None, 3, 12, None),
]


def _loop_model():
    e2i, i2e = _toy_vocab()
    sd = _sd(2, seed=5)
    for e, i in e2i.items():                                         # keys, bars and beats likely: the key rule passes and the grammar has work
        if e.startswith('Key_') or e == 'Bar_None' or e.startswith('Beat_'):
            sd['dec_out_proj.bias'][i] += 3.0
    return _model(2, 8, 'bf16', sd, max_gen_len=96), e2i, i2e


def _host_grammar_on_device_draws(m, e2i, i2e, streams, seed):
    """The method of test_device_loop_equals_host_grammar_on_the_same_draws with the one-launch step as the model step: ops.sample_nucleus on the
    loop's own uniform table, grammar on the host (_LeadSheet)."""
    from test_gpu_stage1_batch import HostStream
    from emo_disentanger_amd import ops, stage1_inference as s1
    cols = list(zip(*streams))
    loop = s1.LeadSheetLoop(m, e2i, i2e, list(cols[0]), representation=list(cols[1]), key_determine=list(cols[2]), max_bars=list(cols[3]),
                            max_events=list(cols[4]), prompt_bars=list(cols[5]), temp=1.2, top_p=0.9, seed=seed, step='one_launch')
    n = loop.n
    hosts = [HostStream(e2i, i2e, *st, loop.L0) for st in streams]
    logits, pos = loop.logits.clone(), loop.L0
    while any(h.status == s1.RUNNING for h in hosts):
        ctr = torch.tensor([min(h.draws, loop.U.shape[0] - 1) for h in hosts], device='cuda')
        u = loop.U.gather(0, ctr.view(1, n)).view(n).contiguous()
        w_main = ops.sample_nucleus(logits, 1.2, 0.9, u).cpu().tolist()
        w_key = ops.sample_nucleus(logits, s1.KEY_TEMP, s1.KEY_TOP_P, u).cpu().tolist()
        for i, h in enumerate(hosts):
            h.step((w_key if h.key_step() else w_main)[i] if h.wants_draw() else None)
        if not any(h.status == s1.RUNNING for h in hosts) or pos >= loop.max_len:
            break
        tok = torch.tensor([h.tok if h.tok is not None else 0 for h in hosts], dtype=torch.long, device='cuda')
        logits = loop.stepper.step(tok).clone()
        pos += 1
    loop.stepper.check_persistent()
    return [(h.status, h.sheet.tokens[:-1] if h.status == s1.DONE else None) for h in hosts]


def test_one_launch_loop_obeys_the_host_grammar_and_replays():
    from emo_disentanger_amd import stage1_inference as s1
    m, e2i, i2e = _loop_model()
    cols = list(zip(*STREAMS6))
    kw = dict(representation=list(cols[1]), key_determine=list(cols[2]), max_bars=list(cols[3]), max_events=list(cols[4]),
              prompt_bars=list(cols[5]), temp=1.2, top_p=0.9, seed=7, step='one_launch')
    got, _ = s1.generate_lead_sheets(m, e2i, i2e, list(cols[0]), use_graph=True, **kw)          # (check_persistent inside run())
    eager, _ = s1.generate_lead_sheets(m, e2i, i2e, list(cols[0]), use_graph=False, **kw)
    again, _ = s1.generate_lead_sheets(m, e2i, i2e, list(cols[0]), use_graph=True, **kw)        # a second loop on the same model, the same seed
    ref = _host_grammar_on_device_draws(m, e2i, i2e, STREAMS6, 7)
    status = lambda r: s1.STUCK if r is None else s1.KEY_ERROR if isinstance(r, ValueError) else s1.DONE if isinstance(r, list) else -1
    ids = lambda rs: [r if isinstance(r, list) else None for r in rs]
    assert [status(r) for r in got] == [st for st, _ in ref]
    assert ids(got) == [x for _, x in ref]
    assert [status(r) for r in eager] == [status(r) for r in got] and ids(eager) == ids(got)
    assert [status(r) for r in again] == [status(r) for r in got] and ids(again) == ids(got)
    assert sum(isinstance(r, list) for r in got) >= 3


def test_one_launch_loop_ends_at_the_last_cache_row_like_the_chain():
    """max_gen_len = 16: streams that never finish reach row 15 and end with the chain's EmoError; one more step — its lengths point past the
    cache — rewrites row 15 of its own (stream, head) and leaves row 0 of every neighbouring (stream, head) bit-unchanged."""
    from emo_disentanger_amd import stage1_inference as s1
    from emo_disentanger_amd._lib import EmoError
    e2i, i2e = _toy_vocab()
    sd = _sd(2, seed=5)
    for e, i in e2i.items():                                         # notes only: no bar, no EOS, no beat — nothing ends a stream but the cache
        if e.startswith('Note_Degree_'):
            sd['dec_out_proj.bias'][i] += 30.0
    m = _model(2, 8, 'bf16', sd, max_gen_len=16)
    primers = [['Emotion_Q1'], ['Emotion_Q2'], ['Emotion_Q3'], ['Emotion_Q4']]      # (a full group: an idle padding stream rewrites its own row 0 every step)
    kw = dict(max_bars=8, max_events=64, temp=1.2, top_p=0.9, representation='remi', key_determine=None, seed=3)
    chain, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, step='chain', **kw)
    loop = s1.LeadSheetLoop(m, e2i, i2e, primers, step='one_launch', **kw)
    row0 = [t[:, :, 0].clone() for t in loop.mem.kc_all + loop.mem.vc_all]
    loop.run()                                                       # (check_persistent inside)
    one = loop.results()
    assert all(isinstance(r, EmoError) for r in chain) and all(isinstance(r, EmoError) for r in one)
    assert [str(r) for r in one] == [str(r) for r in chain] and 'max_gen_len=16' in str(one[0])
    assert int(loop.mem.lens.min()) == 16
    last = [t[:, :, 15].clone() for t in loop.mem.kc_all]
    loop.stepper.step(loop.tok)                                      # lengths 17: the row index is clamped to 15
    torch.cuda.synchronize()
    loop.stepper.check_persistent()
    for a, t in zip(row0, loop.mem.kc_all + loop.mem.vc_all):
        assert torch.equal(a, t[:, :, 0])
    assert any(not torch.equal(a, t[:, :, 15]) for a, t in zip(last, loop.mem.kc_all))      # the clamped row is where the step wrote


@pytest.mark.parametrize('what,build,n', [
    ('bf16', lambda: _model(1, 8, 'fp32'), 4),
    ('d_model 512', lambda: _model(1, 8, 'bf16', d=256), 4),
    ('mem_len', lambda: _model(1, 4096, 'bf16', max_gen_len=32), 4),
    ('1 to 32 streams', lambda: _model(1, 8, 'bf16', max_gen_len=32), 33),
    ('pre_lnorm', lambda: _model(1, 8, 'bf16', pre_lnorm=False), 4),
])
def test_one_launch_step_refuses_what_it_was_not_built_for(what, build, n):
    from emo_disentanger_amd import stage1_inference as s1
    from emo_disentanger_amd._lib import EmoError
    e2i, i2e = _toy_vocab()
    with pytest.raises(EmoError, match=what):
        s1.generate_lead_sheets(build(), e2i, i2e, [['Emotion_Q1']] * n, max_bars=2, max_events=8, representation='remi', step='one_launch')
