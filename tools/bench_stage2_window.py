"""Stage-2 generation PAST the 2048-token window at the benchmark shape (d 512, 12 layers, 8 heads, d_ff 2048, V = 327, bf16, seeded random
weights, the synthetic vocabulary / model / lead sheets of bench_stage2_gen.py, lead sheets long enough that every stream reaches the
window), Performer (128 features) and GPT-2, 32 streams.  After the in-window device loop has handed the streams off, in ONE process:
  device   WindowedLoop (one batched [m, 2048] forward + emo_grammar_step (kind ACC_WINDOW) per draw, a poll every 16 steps): ms per step, accepted draws / s
  host     _resume_windowed on the SAME handed-off streams, one after the other, each capped at --host-draws accepted draws, repeated
           --host-repeats times (same draws every repeat): accepted draws / s per repeat, best and spread
  forward  the bare [32, 2048] eval forward, keep_last_only (what a windowed step cannot go below)
`device_over_host_best` compares the device phase with the host leg's best repeat; `beats_host_by_more_than_spread` says whether the margin
exceeds the host leg's spread.  Prints one JSON line (and writes it to --out).
Arguments: --streams N (32), --bars N (120), --steps N windowed device steps (192), --kinds performer,gpt2, --loop-only (the windowed device
steps alone after the handoff: the run a kernel-trace profile is taken of)."""
import argparse
import contextlib
import copy
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_stage2_gen import D, DFF, H, L, NF, TEMP, TOP_P, V, batch, model, vocab  # noqa: E402


def device_phase(inf, loop, seed, steps):
    wl = inf.WindowedLoop(loop, seed)
    torch.cuda.synchronize()
    wl.run(max_steps=steps)
    acc = wl.accepted_draws()
    return dict(streams=wl.m0, steps=wl.steps, accepted_draws=acc, seconds=round(wl.seconds, 4), ms_per_step=round(1e3 * wl.seconds / wl.steps, 4),
                draws_per_s=round(acc / wl.seconds, 1), rows_first=wl.batch_rows[0], rows_last=wl.batch_rows[-1], poll_every=wl.k)


def host_phase(inf, m, e2i, i2e, loop, seed, cap):
    """_resume_windowed on every handed-off stream in turn (the path AccompanimentLoop.results takes), each stopped after `cap` accepted draws."""
    state = loop.state.cpu().numpy()
    idx = [i for i in range(loop.n) if state[i, inf.ACC_S_STATUS] == inf.ACC_WINDOW]
    streams = [copy.deepcopy(loop.handed_off(i)) for i in idx]
    accepted = [0]
    for s in streams:
        def offer(*a, s=s, f=s.offer, mine=[0]):
            ok = f(*a)
            if ok and not s.stuck:
                accepted[0] += 1
                mine[0] += 1
                if mine[0] >= cap:
                    s.done = True
            return ok
        s.offer = offer
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, s in zip(idx, streams):
        rs = np.random.RandomState([seed, i])
        inf._resume_windowed(m, e2i, i2e, s, loop.max_events, False, TEMP, None, lambda p, rs=rs: inf.nucleus(p, TOP_P, rng=rs))
    sec = time.perf_counter() - t0
    return dict(streams=len(idx), accepted_draws=accepted[0], seconds=round(sec, 4), draws_per_s=round(accepted[0] / sec, 1))


def bare_forward(m, n, W, reps=10):
    tok = torch.randint(0, V - 1, (n, W), device='cuda')
    seg = torch.randint(0, 2, (n, W), device='cuda')
    kw = {'attn_kwargs': {'omit_feature_map_draw': True}} if m.kind == 'performer' else {}
    with torch.no_grad():
        for _ in range(3):
            m(tok, seg_inp=seg, keep_last_only=True, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            m(tok, seg_inp=seg, keep_last_only=True, **kw)
        torch.cuda.synchronize()
    return round(1e3 * (time.perf_counter() - t0) / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--bars', type=int, default=120)
    ap.add_argument('--steps', type=int, default=192)
    ap.add_argument('--host-draws', type=int, default=16)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--kinds', default='performer,gpt2')
    ap.add_argument('--loop-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from emo_disentanger_amd import inference as inf
    torch.cuda.set_device(0)
    e2i, i2e = vocab()
    leads, primers = batch(e2i, args.streams, args.bars)
    W = inf.max_dec_inp_len
    out = {'tool': 'bench_stage2_window', 'shape': dict(d_model=D, n_layer=L, n_head=H, d_ff=DFF, V=V, performer_features=NF, dtype='bf16'),
           'streams': args.streams, 'bars': args.bars, 'window': W, 'temp': TEMP, 'top_p': TOP_P, 'host_draws_per_stream': args.host_draws}
    for kind in args.kinds.split(','):
        m = model(kind, e2i)
        loop = inf.AccompanimentLoop(m, e2i, i2e, leads, primers, temp=TEMP, top_p=TOP_P, seed=1)
        loop.run(use_graph=True)
        r = {'in_window': dict(steps=loop.steps(), persistent=loop.eng.persist is not None, **loop.counts())}
        if r['in_window']['window'] == 0:
            raise SystemExit('no stream reached the window: raise --bars')
        device_phase(inf, loop, 1, 2 * 16)                                  # warm-up (kernel / workspace caches of the [m, W] shapes)
        if args.loop_only:
            r['device'] = device_phase(inf, loop, 1, args.steps)
            out[kind] = r
            continue
        r['device'] = device_phase(inf, loop, 1, args.steps)
        with contextlib.redirect_stdout(sys.stderr):
            host_phase(inf, m, e2i, i2e, loop, 1, 2)                        # warm-up of the [1, W] shapes
            r['host'] = [host_phase(inf, m, e2i, i2e, loop, 1, args.host_draws) for _ in range(args.host_repeats)]
        rates = [h['draws_per_s'] for h in r['host']]
        r['host_best_draws_per_s'], r['host_spread_draws_per_s'] = max(rates), round(max(rates) - min(rates), 1)
        r['device_over_host_best'] = round(r['device']['draws_per_s'] / max(rates), 2)
        r['beats_host_by_more_than_spread'] = bool(r['device']['draws_per_s'] - max(rates) > max(rates) - min(rates))
        r['bare_forward_ms'] = bare_forward(m, r['device']['rows_first'], W)
        r['step_over_bare_forward'] = round(r['device']['ms_per_step'] / r['bare_forward_ms'], 4)
        out[kind] = r
        del loop, m
        torch.cuda.empty_cache()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
