"""Stage-2 accompaniment generation at the benchmark shape (d 512, 12 layers, 8 heads, d_ff 2048, V = 327, bf16, seeded random weights, a
synthetic stage-2 vocabulary, synthetic lead sheets of 8 bars, output-bias nudges so that Track_LeadSheet and Beats occur and pieces
finish), Performer (128 features) and GPT-2, 32 streams: the host loop generate_conditional_batch (NumPy draws and grammar, a host sync per
step) against the device loop generate_accompaniments (emo_grammar_step, kind ACC, + the one-launch engine step, hipGraph replays), and the bare
engine step replayed the same way over the same positions.  Prints one JSON line.
`ms_per_step` of the device loop is run() as a caller sees it (eager first step and graph capture included); `replay_ms_per_step` is the
replay phase alone, the figure compared with the bare step (`device_over_bare`).
Arguments: --streams N (default 32), --bars N (default 8), --kinds performer,gpt2, --loop-only (the device loops alone: the run a
kernel-trace profile is taken of)."""
import argparse
import contextlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

D, L, H, DFF, V, NF = 512, 12, 8, 2048, 327, 128
TEMP, TOP_P = 1.2, 0.9


def vocab():
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4')] + ['Key_%s' % k for k in ('C', 'a', 'G', 'e', 'F', 'd')]
             + ['Tempo_%d' % t for t in range(60, 180, 10)] + ['Track_LeadSheet', 'Track_Full', 'Bar_None'] + ['Beat_%d' % i for i in range(16)]
             + ['Chord_%d_%d' % (i // 8, i % 8) for i in range(96)])
    names += ['Note_Pitch_%d' % i for i in range(V - 2 - len(names))] + ['EOS_None', 'PAD_None']
    assert len(names) == V
    return {e: i for i, e in enumerate(names)}, dict(enumerate(names))


def model(kind, e2i):
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        if kind == 'performer':
            m = MusicPerformer(V, L, H, D, DFF, D, favor_feature_dims=NF, use_segment_emb=True, n_segment_types=2, compute_dtype='bf16', redraw='fixed')
        else:
            m = MusicGPT2(V, L, H, D, DFF, D, use_segment_emb=True, n_segment_types=2, dropout=0.1, compute_dtype='bf16')
    with torch.no_grad():                          # a bar ends after ~20 events, Beats are common, EOS shows up (and is rejected before the end)
        b = m.dec_out_proj.bias
        b[e2i['Track_LeadSheet']] += 3.5
        b[e2i['EOS_None']] += 1.0
        for k in range(16):
            b[e2i['Beat_%d' % k]] += 2.0
    return m.cuda().eval()


def batch(e2i, n, bars, seed=1):
    rs = np.random.RandomState(seed)
    beats = [e2i['Beat_%d' % k] for k in range(0, 16, 4)]
    chords = [e2i['Chord_%d_%d' % (i // 8, i % 8)] for i in range(96)]
    leads = []
    for _ in range(n):
        lead = []
        for _ in range(bars):
            bar = [e2i['Bar_None']]
            for bt in sorted(rs.choice(beats, size=rs.randint(1, 4), replace=False).tolist()):
                bar += [bt, int(rs.choice(chords))]
            lead.append(bar)
        leads.append(lead)
    primers = [[e2i['Emotion_Q%d' % (1 + i % 4)], e2i[['Key_C', 'Key_a', 'Key_G', 'Key_e'][i % 4]], e2i['Tempo_110']] for i in range(n)]
    return leads, primers


def host_loop(inf, m, e2i, i2e, leads, primers):
    """generate_conditional_batch, with its engine steps and accepted samples counted."""
    steps, accepted = [0], [0]
    orig_make, orig_offer = inf.make_engine, inf._Stream.offer

    def make(model, n, **kw):
        eng = orig_make(model, n, **kw)
        f = eng.step

        def step(*a, **k):
            steps[0] += 1
            return f(*a, **k)
        eng.step = step
        return eng

    def offer(self, *a):
        ok = orig_offer(self, *a)
        accepted[0] += int(ok and not self.stuck)
        return ok
    inf.make_engine, inf._Stream.offer = make, offer
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = inf.generate_conditional_batch(m, e2i, i2e, leads, primers, temp=TEMP, top_p=TOP_P, seeds=list(range(len(leads))))
        sec = time.perf_counter() - t0
    finally:
        inf.make_engine, inf._Stream.offer = orig_make, orig_offer
    tls = e2i['Track_LeadSheet']
    done = sum(r.count(tls) == len(ld) for r, ld in zip(res, leads))
    return dict(steps=steps[0], accepted_tokens=accepted[0], seconds=round(sec, 4), ms_per_step=round(1e3 * sec / steps[0], 4),
                tokens_per_s=round(accepted[0] / sec, 1), finished=done, not_finished=len(res) - done)


def device_loop(inf, m, e2i, i2e, leads, primers, seed):
    loop = inf.AccompanimentLoop(m, e2i, i2e, leads, primers, temp=TEMP, top_p=TOP_P, seed=seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(use_graph=True)
    sec = time.perf_counter() - t0
    steps, acc = loop.steps(), loop.accepted_tokens()
    rs, rsec = loop.replayed
    out = dict(steps=steps, accepted_tokens=acc, seconds=round(sec, 4), ms_per_step=round(1e3 * sec / steps, 4), tokens_per_s=round(acc / sec, 1),
               replay_steps=rs, replay_ms_per_step=round(1e3 * rsec / max(rs, 1), 4), persistent=loop.eng.persist is not None, L0=loop.L0)
    out.update(loop.counts())
    return out, loop


def bare_step(inf, m, e2i, i2e, leads, primers, steps, k=16):
    """The engine step alone (dev_pos, static logits), k steps per hipGraph replay, the count polled once per replay as the device loop does,
    over the positions the device loop's replays ran (L0 + 1 ...)."""
    loop = inf.AccompanimentLoop(m, e2i, i2e, leads, primers, temp=TEMP, top_p=TOP_P, seed=0)
    eng = loop.eng

    def one():
        eng.step(loop.tok, loop.segv, dev_pos=True, logits_out=loop.logits)
    from emo_disentanger_amd.replay import StepReplayer, replay_plan
    rp = StepReplayer(one, loop.dev, k)
    with torch.no_grad():
        one()
        torch.cuda.synchronize()
        counts, many = replay_plan(0, steps, k)
        graphs = {1: rp.capture(1)}
        if many:
            graphs[k] = rp.capture(k)
        main, s = torch.cuda.current_stream(), rp.stream
        t0 = time.perf_counter()
        with torch.cuda.stream(s):
            for c in counts:
                graphs[c].replay()
                eng.check_persistent() if eng.persist is not None else None
                int(loop.running.item())
        main.wait_stream(s)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
    return round(1e3 * sec / steps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--bars', type=int, default=8)
    ap.add_argument('--kinds', default='performer,gpt2')
    ap.add_argument('--loop-only', action='store_true')
    args = ap.parse_args()
    from emo_disentanger_amd import inference as inf
    torch.cuda.set_device(0)
    e2i, i2e = vocab()
    leads, primers = batch(e2i, args.streams, args.bars)
    out = {'tool': 'bench_stage2_gen', 'shape': dict(d_model=D, n_layer=L, n_head=H, d_ff=DFF, V=V, performer_features=NF, dtype='bf16'),
           'streams': args.streams, 'bars': args.bars, 'temp': TEMP, 'top_p': TOP_P}
    for kind in args.kinds.split(','):
        m = model(kind, e2i)
        wl, wp = batch(e2i, args.streams, 1, seed=99)
        inf.generate_accompaniments(m, e2i, i2e, wl, wp, temp=TEMP, top_p=TOP_P, seed=99)             # warm-up (kernels, workspaces, graphs)
        if args.loop_only:
            dev, _ = device_loop(inf, m, e2i, i2e, leads, primers, seed=1)
            out[kind] = {'device': dev}
            continue
        with contextlib.redirect_stdout(sys.stderr):
            inf.generate_conditional_batch(m, e2i, i2e, wl, wp, temp=TEMP, top_p=TOP_P)                 # warm-up of the host loop
        r = {'host': host_loop(inf, m, e2i, i2e, leads, primers)}
        r['device'], loop = device_loop(inf, m, e2i, i2e, leads, primers, seed=1)
        r['bare_step_ms'] = bare_step(inf, m, e2i, i2e, leads, primers, r['device']['replay_steps'])
        r['device_over_bare'] = round(r['device']['replay_ms_per_step'] / r['bare_step_ms'], 4)
        r['device_over_bare_incl_capture'] = round(r['device']['ms_per_step'] / r['bare_step_ms'], 4)
        r['device_over_host_tokens_per_s'] = round(r['device']['tokens_per_s'] / r['host']['tokens_per_s'], 2)
        r['host_over_device_ms_per_step'] = round(r['host']['ms_per_step'] / r['device']['ms_per_step'], 2)
        out[kind] = r
        del loop, m
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
