"""GPU: stage-1 lead sheets in lock-step batches — generate_plain_xl_batch (NumPy grammar and sampling per stream, reference-exact),
the device grammar step emo_txl_grammar_step, PlainTransformer.decode_step, the graph-replayed device loop generate_lead_sheets and the
stage-1 command line."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')


def _fixture(dtype='fp32'):
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    from oracle.txl_ref import make_state_dict_txl
    g = json.load(open(os.path.join(G, 'txl_generate.json')))
    c = g['model']
    e2i = {e: i for i, e in enumerate(g['events'])}
    i2e = {i: e for e, i in e2i.items()}
    sd = make_state_dict_txl(c['V'], c['L'], c['H'], c['d'], c['dff'], seed=c['seed'], scale=c['scale'])
    m = PlainTransformer(c['d'], c['V'], c['L'], c['H'], c['d'], c['dff'], c['T'], c['T'], dec_dropout=0.1, pre_lnorm=True, compute_dtype=dtype)
    m.load_state_dict(sd)
    return g, m.cuda().eval(), e2i, i2e


def test_batch_reproduces_the_reference_traces_in_one_call(monkeypatch):
    # the four recorded runs of the REAL reference loop as four streams of ONE call, each with RandomState(its seed): same sampled words
    # (incl. the rejected ones) and the same output; seed 1 ends in the key rule's ValueError
    from emo_disentanger_amd import stage1_inference as s1
    g, m, e2i, i2e = _fixture()
    runs = g['runs']
    kws = [r['kw'] for r in runs]
    per = lambda k, d: [kw.get(k, d) for kw in kws]
    fresh = {r['seed']: np.random.RandomState(r['seed']).get_state() for r in runs}
    rec = {}
    orig = s1.nucleus

    def spy(probs, p, rng=None):
        if id(rng) not in rec:                  # first draw of a stream: its generator is still in its seeded state
            st = rng.get_state()
            seed = [s for s, f in fresh.items() if np.array_equal(f[1], st[1]) and f[2] == st[2]]
            assert len(seed) == 1
            rec[id(rng)] = (seed[0], [], rng)
        w = orig(probs, p, rng=rng)
        rec[id(rng)][1].append(int(w))
        return w
    monkeypatch.setattr(s1, 'nucleus', spy)
    res, _ = s1.generate_plain_xl_batch(m, e2i, i2e, per('primer', None), max_bars=per('max_bars', 160), max_events=per('max_events', 2048),
                                        temp=1.2, top_p=0.9, prompt_bars=per('prompt_bars', None), representation=per('representation', 'functional'),
                                        key_determine=per('key_determine', None), seeds=[r['seed'] for r in runs])
    sampled = {seed: lst for seed, lst, _ in rec.values()}
    for i, run in enumerate(runs):
        if run['error'] is not None:
            assert isinstance(res[i], ValueError) and run['error'] in str(res[i])
        else:
            assert res[i] == run['generated'], run['seed']
        assert sampled[run['seed']] == run['sampled'], run['seed']


def _scripted(e2i, script, seed):
    """sampler: the scripted events first (forced key mismatches, PADs, non-keys), then nucleus(probs, 0.9) with RandomState(seed)."""
    from emo_disentanger_amd import stage1_inference as s1
    todo, rs = [e2i[e] for e in script], np.random.RandomState(seed)

    def pick(probs):
        return todo.pop(0) if todo else s1.nucleus(probs, 0.9, rng=rs)
    return pick


MIXED = [  # primer, representation, key_determine, max_bars, max_events, prompt_bars, scripted first samples
    (['Emotion_Q1'], 'functional', 'rule', 3, 60, None, ['Key_a', 'Key_e', 'Key_C']),
    (['Emotion_Q2'], 'functional', 'rule', 4, 50, None, ['Key_G', 'Key_a', 'PAD_None']),
    (['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M'], 'functional', None, 3, 70, 1, ['PAD_None', 'PAD_None']),
    (None, 'remi', None, 2, 40, None, []),
    (['Emotion_Negative'], 'functional', 'rule', 4, 60, None, ['Bar_None']),
    (['Emotion_Positive'], 'functional', None, 3, 60, None, ['Beat_3', 'Beat_1', 'Beat_1']),
]


def test_mixed_batch_equals_single_stream_runs():
    from emo_disentanger_amd import stage1_inference as s1
    _, m, e2i, i2e = _fixture()
    cols = list(zip(*MIXED))
    res, _ = s1.generate_plain_xl_batch(m, e2i, i2e, list(cols[0]), representation=list(cols[1]), key_determine=list(cols[2]), max_bars=list(cols[3]),
                                        max_events=list(cols[4]), prompt_bars=list(cols[5]), temp=1.2, top_p=0.9,
                                        samplers=[_scripted(e2i, sc, 40 + i) for i, sc in enumerate(cols[6])])
    for i, (primer, rep, kd, mb, me, pb, sc) in enumerate(MIXED):
        try:
            single, _ = s1.generate_plain_xl(m, e2i, i2e, max_bars=mb, max_events=me, primer=primer, temp=1.2, top_p=0.9, prompt_bars=pb,
                                             representation=rep, key_determine=kd, sampler=_scripted(e2i, sc, 40 + i))
        except ValueError as e:
            assert isinstance(res[i], ValueError) and str(res[i]) == str(e), i
            continue
        assert res[i] == single, i
    assert isinstance(res[4], ValueError)


class HostStream:
    """Host restatement of one stream of emo_txl_grammar_step on _LeadSheet (the grammar of generate_plain_xl)."""

    def __init__(self, e2i, i2e, primer, rep, kd, mb, me, pb, L0):
        from emo_disentanger_amd import stage1_inference as s1
        self.s1, self.i2e = s1, i2e
        self.sheet = s1._LeadSheet(e2i, primer, pb, mb, me)
        self.plen, self.feed, self.draws, self.tok = len(self.sheet.tokens), L0, 0, None
        self.keyed, self.rule = rep in ('functional', 'key'), kd == 'rule'
        self.status = s1.RUNNING if self.sheet.open() else s1.DONE

    def wants_draw(self):
        return self.status == self.s1.RUNNING and self.feed >= self.plen

    def key_step(self):
        return self.keyed and len(self.sheet.tokens) == 1

    def step(self, word=None):
        s1, sh = self.s1, self.sheet
        if self.status != s1.RUNNING:
            return
        if self.feed < self.plen:
            self.tok = sh.tokens[self.feed]
            self.feed += 1
            return
        self.draws += 1
        try:
            s1._draw(sh, np.zeros(len(self.i2e), np.float32), lambda probs, p: word, self.i2e, self.keyed, self.rule, 1.0, 0.9)
        except ValueError:
            self.status = s1.KEY_ERROR
            return
        if sh.stuck:
            self.status = s1.STUCK
        elif not sh.open():
            self.status = s1.DONE
        elif sh.accepted == 0:
            self.tok, self.feed = sh.tokens[0], 1
        else:
            self.tok = sh.tokens[-1]

    def state(self):
        s1, sh = self.s1, self.sheet
        return {s1.S_STATUS: self.status, s1.S_LEN: len(sh.tokens), s1.S_ACCEPTED: sh.accepted, s1.S_BEAT: sh.beat, s1.S_BARS: sh.bars,
                s1.S_FAILED: sh.rejected_in_a_row, s1.S_DRAWS: self.draws}


UNIT = [  # primer, representation, key_determine, max_bars, max_events, prompt_bars, the words the forced logits pick, in order
    (['Emotion_Q1'], 'functional', None, 4, 100, None, ['Key_C', 'Bar_None', 'Beat_5', 'Beat_3', 'Beat_6', 'Note_Degree_1', 'Bar_None', 'Beat_1',
                                                       'Bar_None', 'Beat_0', 'Bar_None']),                                    # beat regression, bars
    (['Emotion_Positive'], 'remi', None, 8, 600, None, ['Bar_None', 'Beat_7'] + ['Beat_0'] * 256),                            # stuck
    (['Emotion_Q2'], 'functional', None, 4, 100, None, ['PAD_None', 'Key_a', 'PAD_None', 'Chord_I_M', 'EOS_None']),           # PAD, EOS
    (None, 'remi', None, 2, 100, None, ['Bar_None', 'Beat_0', 'Bar_None']),                                                    # max_bars
    (['Emotion_Negative'], 'functional', None, 8, 4, None, ['Key_e', 'Note_Octave_4', 'Note_Degree_3', 'Note_Duration_2']),  # max_events
    (['Emotion_Q1'], 'functional', 'rule', 4, 100, None, ['Key_a', 'Key_e', 'Key_G', 'Bar_None', 'EOS_None']),                # key mismatch
    (['Emotion_Q2'], 'functional', 'rule', 4, 100, None, ['Chord_I_M']),                                                       # non-Key
    (['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M'], 'functional', 'rule', 4, 100, 1,
     ['PAD_None', 'Beat_2', 'Beat_1', 'EOS_None']),                                                                            # primer re-feed
    (None, 'remi', 'rule', 4, 100, None, ['Key_C', 'Beat_3', 'EOS_None']),                                                    # remi: no key step
]


def test_grammar_kernel_matches_the_host_grammar_step_by_step():
    from emo_disentanger_amd import ops, stage1_inference as s1
    g, _, e2i, i2e = _fixture()
    V, n, dev = len(i2e), len(UNIT), 'cuda'
    L0 = min(1 if p is None else len(p) for p, *_ in UNIT)
    hosts = [HostStream(e2i, i2e, p, rep, kd, mb, me, pb, L0) for p, rep, kd, mb, me, pb, _ in UNIT]
    scripts = [[e2i[w] for w in u[-1]] for u in UNIT]
    flags, beat = s1.event_tables(i2e, V)
    W = 700
    seq = np.zeros((n, W), np.int64)
    params = np.zeros((n, 8), np.int32)
    state = np.zeros((n, 8), np.int32)
    for i, (h, u) in enumerate(zip(hosts, UNIT)):
        seq[i, :h.plen] = h.sheet.tokens
        params[i, :6] = u[3], u[4], h.plen, h.keyed, h.rule, s1.emotion_mode(i2e, h.sheet.tokens[0])
        state[i, [s1.S_STATUS, s1.S_LEN, s1.S_BARS, s1.S_FEED]] = h.status, h.plen, h.sheet.bars, L0
    T = lambda a: torch.from_numpy(a).to(dev)
    seq_d, params_d, state_d = T(seq), T(params), T(state)
    ev_flags, ev_beat = T(flags), T(beat)
    running = torch.tensor([sum(h.status == s1.RUNNING for h in hosts)], dtype=torch.int32, device=dev)
    U = torch.rand(400, n, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    tok = torch.full((n,), -1, dtype=torch.long, device=dev)
    steps = 0
    while any(h.status == s1.RUNNING for h in hosts):
        logits = np.zeros((n, V), np.float32)
        words = [None] * n
        for i, h in enumerate(hosts):
            if h.wants_draw():
                words[i] = scripts[i][h.draws]
                logits[i, words[i]] = 60.0                     # one-hot: the nucleus keeps one candidate whatever u is
        ops.txl_grammar_step(T(logits), 1.2, 0.9, 1.1, 0.97, U, ev_flags, ev_beat, params_d, state_d, seq_d, tok, running)
        for i, h in enumerate(hosts):
            h.step(words[i])
        st, sq, tk = state_d.cpu().numpy(), seq_d.cpu().numpy(), tok.cpu().numpy()
        for i, h in enumerate(hosts):
            for k, v in h.state().items():
                assert st[i, k] == v, (steps, i, k, st[i].tolist())
            assert sq[i, :len(h.sheet.tokens)].tolist() == h.sheet.tokens, (steps, i)
            if h.status == s1.RUNNING:
                assert tk[i] == h.tok and st[i, s1.S_FEED] == h.feed, (steps, i)
        assert int(running.item()) == sum(h.status == s1.RUNNING for h in hosts)
        steps += 1
        assert steps < 400
    want = [s1.DONE, s1.STUCK, s1.DONE, s1.DONE, s1.DONE, s1.DONE, s1.KEY_ERROR, s1.DONE, s1.DONE]
    assert [h.status for h in hosts] == want
    assert [h.draws for h in hosts] == [len(s) for s in scripts]          # every scripted word was drawn, nothing more


def test_a_prepared_grammar_block_reused_over_steps_equals_the_one_shot_wrapper():
    # three streams: 0 finished before the first step, 1 still feeding its primer (4 steps, then draws), 2 drawing from the first step with its draw
    # counter at 4 of a uniform table of 8 rows: its fifth step finds the table used up -> OVERFLOW.  A GrammarStep filled once and launched six
    # times leaves, word for word, what ops.txl_grammar_step (a fresh block per call) leaves on its own copies of the same tensors.
    from emo_disentanger_amd import ops, stage1_inference as s1
    g, _, e2i, i2e = _fixture()
    V, n, W, dev = len(i2e), 3, 16, 'cuda'
    primers = [['Emotion_Q2'], ['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M'], ['Emotion_Q1']]
    flags, beat = s1.event_tables(i2e, V)
    seq, params, state = np.zeros((n, W), np.int64), np.zeros((n, 8), np.int32), np.zeros((n, 8), np.int32)
    for i, p in enumerate(primers):
        ids = [e2i[e] for e in p]
        seq[i, :len(ids)] = ids
        params[i, :6] = 8, 100, len(ids), 1, 0, s1.emotion_mode(i2e, ids[0])
        state[i, [s1.S_STATUS, s1.S_LEN, s1.S_FEED]] = s1.RUNNING, len(ids), 1
    state[0, s1.S_STATUS], state[2, s1.S_DRAWS] = s1.DONE, 4
    T = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    shared = dict(u_steps=torch.rand(8, n, device=dev, generator=torch.Generator(device=dev).manual_seed(5)), ev_flags=T(flags), ev_beat=T(beat),
                  params=T(params))
    fresh = lambda: dict(state=T(state), seq=T(seq), tok_out=torch.full((n,), -1, dtype=torch.long, device=dev),      # noqa: E731
                         running=torch.tensor([2], dtype=torch.int32, device=dev))
    one, blk = fresh(), fresh()
    logits = torch.randn(6, n, V, device=dev, generator=torch.Generator(device=dev).manual_seed(6)) * 2.0
    logits[:, :, [e2i['EOS_None'], e2i['Bar_None']]] = -60.0          # no stream ends on its own within the six steps
    lg = torch.empty(n, V, device=dev)
    args, held = ops.GrammarStep(kind=ops.GRAMMAR_TXL), {}
    ops.block_set(args, held, n_rows=n, n_token=V, ld_u=n, temperature=1.2, top_p=0.9, key_temperature=1.1, key_top_p=0.97, logits=lg, **shared, **blk)
    for t in range(6):
        lg.copy_(logits[t])
        ops.txl_grammar_step(lg, 1.2, 0.9, 1.1, 0.97, shared['u_steps'], shared['ev_flags'], shared['ev_beat'], shared['params'], one['state'],
                             one['seq'], one['tok_out'], one['running'])
        ops.grammar_step(args)
        for k in one:
            assert torch.equal(one[k], blk[k]), (t, k, one[k].tolist(), blk[k].tolist())
    st = blk['state'].cpu().numpy()
    assert st[:, s1.S_STATUS].tolist() == [s1.DONE, s1.RUNNING, s1.OVERFLOW] and int(blk['running'].item()) == 1
    assert st[:, s1.S_DRAWS].tolist() == [0, 2, 8] and st[1, s1.S_FEED] >= 1 and (blk['tok_out'].cpu().numpy()[1:] >= 0).all()


STREAMS16 = [  # primer, representation, key_determine, max_bars, max_events, prompt_bars
    (['Emotion_%s' % e], 'functional', kd, mb, me, None) for e, kd, mb, me in
    [('Q1', None, 3, 60), ('Q2', 'rule', 4, 50), ('Positive', None, 2, 40), ('Negative', 'rule', 3, 70), ('Q1', 'rule', 3, 60),
     ('Q2', None, 4, 80), ('Positive', 'rule', 3, 60), ('Negative', None, 2, 30), ('Q1', None, 5, 90), ('Q2', 'rule', 3, 60)]
] + [
    (['Emotion_Positive', 'Key_C', 'Bar_None', 'Beat_0', 'Chord_I_M'], 'functional', None, 3, 70, 1),
    (['Emotion_Negative', 'Key_a', 'Bar_None'], 'functional', 'rule', 4, 60, 1),
    (None, 'remi', None, 2, 40, None), (None, 'remi', None, 3, 60, None), (['Emotion_Q1'], 'remi', None, 3, 60, None),
    (['Emotion_Q2'], 'functional', None, 3, 12, None),
]


def _host_device_draw_loop(m, e2i, i2e, streams, seed):
    """decode_step + ops.sample_nucleus on the device loop's own uniform table, grammar on the host (_LeadSheet)."""
    from emo_disentanger_amd import ops, stage1_inference as s1
    cols = list(zip(*streams))
    loop = s1.LeadSheetLoop(m, e2i, i2e, list(cols[0]), representation=list(cols[1]), key_determine=list(cols[2]), max_bars=list(cols[3]),
                            max_events=list(cols[4]), prompt_bars=list(cols[5]), temp=1.2, top_p=0.9, seed=seed)
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
        logits = m.decode_step(tok, loop.mem)
        pos += 1
    out = []
    for h in hosts:
        out.append((h.status, h.sheet.tokens[:-1] if h.status == s1.DONE else None))
    return out


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_device_loop_equals_host_grammar_on_the_same_draws(dtype):
    from emo_disentanger_amd import stage1_inference as s1
    _, m, e2i, i2e = _fixture(dtype)
    cols = list(zip(*STREAMS16))
    kw = dict(representation=list(cols[1]), key_determine=list(cols[2]), max_bars=list(cols[3]), max_events=list(cols[4]),
              prompt_bars=list(cols[5]), temp=1.2, top_p=0.9, seed=7)
    got, _ = s1.generate_lead_sheets(m, e2i, i2e, list(cols[0]), use_graph=True, **kw)
    eager, _ = s1.generate_lead_sheets(m, e2i, i2e, list(cols[0]), use_graph=False, **kw)
    ref = _host_device_draw_loop(m, e2i, i2e, STREAMS16, 7)
    status = lambda r: s1.STUCK if r is None else s1.KEY_ERROR if isinstance(r, ValueError) else s1.DONE if isinstance(r, list) else -1
    assert [status(r) for r in got] == [st for st, _ in ref]
    assert [r if isinstance(r, list) else None for r in got] == [ids for _, ids in ref]
    assert [status(r) for r in eager] == [status(r) for r in got]
    assert [r if isinstance(r, list) else None for r in eager] == [r if isinstance(r, list) else None for r in got]
    assert sum(isinstance(r, list) for r in got) >= 8


def _synthetic_vocab():
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative')]
             + ['Key_%s' % k for k in ('C', 'C#', 'D', 'D#', 'E', 'F', 'F#', 'G', 'G#', 'A', 'A#', 'B')]
             + ['Key_%s' % k for k in ('c', 'c#', 'd', 'd#', 'e', 'f', 'f#', 'g', 'g#', 'a', 'a#', 'b')]
             + ['Bar_None'] + ['Beat_%d' % i for i in range(16)] + ['Tempo_%d' % t for t in range(60, 180, 10)])
    names += ['Chord_%d_%d' % (i // 8, i % 8) for i in range(88)]
    names += ['Note_Degree_%d' % i for i in range(200 - 2 - len(names))] + ['EOS_None', 'PAD_None']
    assert len(names) == 200
    return {e: i for i, e in enumerate(names)}, dict(enumerate(names))


def test_full_shape_device_loop_obeys_the_grammar():
    from emo_disentanger_amd import stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    torch.manual_seed(0)
    m = PlainTransformer(512, 200, 12, 8, 512, 2048, 512, 512, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16').cuda().eval()
    e2i, i2e = _synthetic_vocab()
    emos = ['Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative']
    primers = [['Emotion_%s' % emos[i % 6]] for i in range(32)]
    kw = dict(max_bars=16, max_events=512, temp=1.2, top_p=0.97, representation='functional', key_determine=None, seed=5)
    a, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **kw)
    b, _ = s1.generate_lead_sheets(m, e2i, i2e, primers, **kw)
    assert a == b
    for ids in a:
        assert ids is None or isinstance(ids, list), ids
        if ids is None:
            continue
        assert len(ids) <= 512
        beat, bars = 0, 0
        for w in ids[1:]:
            e = i2e[w]
            assert e != 'PAD_None'
            if 'Beat' in e:
                assert s1.beat_position(e) >= beat
                beat = s1.beat_position(e)
            if 'Bar' in e:
                bars, beat = bars + 1, 0
        assert bars <= 16
    assert sum(isinstance(r, list) for r in a) >= 16


def test_command_line_writes_lead_sheets_that_stage2_reads(tmp_path):
    import yaml
    from emo_disentanger_amd import inference, stage1_inference as s1
    from oracle.txl_ref import make_state_dict_txl
    g = json.load(open(os.path.join(G, 'txl_generate.json')))
    events = [e for e in g['events'] if e != 'PAD_None']
    vocab = tmp_path / 'dictionary.pkl'
    pickle.dump(({e: i for i, e in enumerate(events)}, {i: e for i, e in enumerate(events)}), open(vocab, 'wb'))
    V = len(events) + 1
    sd = make_state_dict_txl(V, 2, 4, 64, 128, seed=3, scale=2.0)
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
             '-n', '2', '--streams', '3', '--dtype', 'fp32'])
    files = sorted(os.listdir(out))
    assert files and all(f.startswith('samp_0') and f.endswith('_roman.txt') and ('Positive' in f or 'Negative' in f) for f in files)
    e2i, _, _ = s1.read_vocab(str(vocab))
    for f in files:
        lines = open(out / f).read().splitlines()
        assert not any(x.startswith('Emotion_') for x in lines[:1])
        key, bars = inference.read_lead_sheet(str(out / f), e2i)
        assert key.startswith('Key_') and bars and all(b[0] == e2i['Bar_None'] for b in bars)
