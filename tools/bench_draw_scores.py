"""What recording the scores at the draw costs, and what it saves.
1. The grammar launch (emo_grammar_step) of the three kinds with the three per-token outputs (tok_logp / tok_rank / tok_entropy) against the
   same launch with NULL pointers, at the shapes of bench_stage2_gen.py / bench_stage1_gen.py: 32 streams, V = 327 (ACC, ACC_WINDOW with a
   2048-token window) and V = 200 (TXL), randn x 3 logits, every stream drawing in every launch.  Both variants run the same launches from the
   same start state, interleaved; the figure is the median over the repeats of the mean launch time of a back-to-back batch.
2. best_of = 4 ranked by the scoring forward ('forward') against ranked by the recorded figures ('draws'): generate_lead_sheets (8 primers x 4)
   and generate_accompaniments (8 lead sheets x 4, GPT-2) end to end, at the same benchmark shapes.
Both parts run in one process; writes profiles/draw_scores_bench.json and prints it as one JSON line.  No pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402

TXL, ACC, WIN = 0, 1, 2
NAMES = {TXL: 'txl', ACC: 'acc', WIN: 'acc_window'}
N = 32


def rig(ops, kind, with_scores, launches, seed=0):
    """32 streams that draw in every launch (every event plain but PAD, which the random logits all but never give), the argument block."""
    V = 200 if kind == TXL else 327
    W = 2048
    L = W if kind == WIN else 3
    width = L + launches + 8
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(seed)
    flags = torch.zeros(V, dtype=torch.int32, device=dev)
    flags[V - 1] = 4
    params, state = torch.zeros(N, 8, dtype=torch.int32, device=dev), torch.zeros(N, 8, dtype=torch.int32, device=dev)
    state[:, 1] = L
    if kind == TXL:
        params[:, 0], params[:, 1], params[:, 2], state[:, 6] = 1 << 20, 1 << 20, L, L
    else:
        params[:, 0], params[:, 1], params[:, 4], state[:, 2] = 1 << 20, 1 << 20, 1, L
    t = dict(logits=(torch.randn(N, V, device=dev, generator=g) * 3).contiguous(), u_steps=torch.rand(4 * launches, N, device=dev, generator=g),
             ev_flags=flags, ev_beat=torch.zeros(V, dtype=torch.int32, device=dev), params=params, state=state,
             seq=torch.zeros(N, width, dtype=torch.int64, device=dev), running=torch.tensor([N], dtype=torch.int32, device=dev))
    num = dict(n_rows=N, n_token=V, ld_u=N, temperature=1.2, top_p=0.9)
    if kind == TXL:
        num.update(key_temperature=1.1, key_top_p=0.97)
        t.update(tok_out=torch.zeros(N, dtype=torch.int64, device=dev))
    else:
        t.update(segs=torch.zeros(N, width, dtype=torch.int64, device=dev), lead_tok=torch.zeros(4, dtype=torch.int64, device=dev),
                 lead_off=torch.tensor([0, 2, 4], dtype=torch.int32, device=dev))
        if kind == ACC:
            num.update(max_len=width + 8, pad=V - 1)
            t.update(tok_out=torch.zeros(N, dtype=torch.int64, device=dev), seg_out=torch.zeros(N, dtype=torch.int64, device=dev))
        else:
            num.update(window=W)
            t.update(win_tok=torch.zeros(N, W, dtype=torch.int64, device=dev), win_seg=torch.zeros(N, W, dtype=torch.int64, device=dev))
    if with_scores:
        t.update(ops.draw_score_tables(t['seq']))
    args, held = ops.GrammarStep(kind=kind), {}
    ops.block_set(args, held, **num, **t)
    return args, held, t


def time_launches(ops, kind, with_scores, launches, warmup):
    args, held, t = rig(ops, kind, with_scores, launches + warmup)
    for _ in range(warmup):
        ops.grammar_step(args)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        ops.grammar_step(args)
    b.record()
    torch.cuda.synchronize()
    accepted = int(t['state'][:, 2 if kind == TXL else 7].sum().item())
    assert int(t['running'].item()) == N, 'a stream left RUNNING: the launches timed are not all drawing launches'
    return 1e3 * a.elapsed_time(b) / launches, accepted


def launch_cost(ops, launches, repeats, warmup):
    out = {}
    for kind in (ACC, WIN, TXL):
        plain, scored = [], []
        for _ in range(repeats):
            us0, acc0 = time_launches(ops, kind, False, launches, warmup)
            us1, acc1 = time_launches(ops, kind, True, launches, warmup)
            assert acc0 == acc1                                   # the same draws either way
            plain.append(us0)
            scored.append(us1)
        p, s = statistics.median(plain), statistics.median(scored)
        out[NAMES[kind]] = dict(V=200 if kind == TXL else 327, streams=N, launches=launches, repeats=repeats, accepted_per_run=acc1,
                                us_without=round(p, 2), us_with=round(s, 2), us_added=round(s - p, 2),
                                us_without_min_max=[round(min(plain), 2), round(max(plain), 2)],
                                us_with_min_max=[round(min(scored), 2), round(max(scored), 2)])
    return out


def best_of_cost(repeats):
    import bench_stage1_gen as b1
    import bench_stage2_gen as b2
    from emo_disentanger_amd import inference as inf, stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    out = {}
    torch.manual_seed(0)
    m = PlainTransformer(b1.D, b1.V, b1.L, b1.H, b1.D, b1.DFF, b1.TGT, b1.TGT, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16').cuda().eval()
    e2i, i2e = b1.vocab()
    emos = ['Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative']
    primers = [['Emotion_%s' % emos[i % 6]] for i in range(8)]
    kw = dict(max_bars=128, max_events=256, temp=1.2, top_p=0.97, representation='functional', key_determine=None, seed=1, best_of=4)
    runs = {'stage1': lambda by: s1.generate_lead_sheets(m, e2i, i2e, primers, best_by=by, **kw)}
    e2, i2 = b2.vocab()
    m2 = b2.model('gpt2', e2)
    leads, pr2 = b2.batch(e2, 8, 4)
    runs['stage2_gpt2'] = lambda by: inf.generate_accompaniments(m2, e2, i2, leads, pr2, temp=b2.TEMP, top_p=b2.TOP_P, seed=1, best_of=4, best_by=by)
    for name, run in runs.items():
        rec = {}
        for by in ('forward', 'draws'):
            run(by)                                               # warm-up (kernels, workspaces, graph capture paths)
            secs = []
            for _ in range(repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = run(by)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
            picks = res[2]
            rec[by] = dict(seconds=round(statistics.median(secs), 4), seconds_all=[round(x, 4) for x in secs], chosen=[p['chosen'] for p in picks],
                           nll_mean_chosen=[None if p['nll_mean'][p['chosen']] != p['nll_mean'][p['chosen']] else round(p['nll_mean'][p['chosen']], 4)
                                            for p in picks])
        rec['same_pick'] = sum(a == b for a, b in zip(rec['forward']['chosen'], rec['draws']['chosen']))
        rec['pieces'], rec['best_of'] = len(rec['forward']['chosen']), 4
        rec['seconds_saved'] = round(rec['forward']['seconds'] - rec['draws']['seconds'], 4)
        out[name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--gen-repeats', type=int, default=3)
    ap.add_argument('--launch-only', action='store_true')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'draw_scores_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import ops
    torch.cuda.set_device(0)
    out = {'tool': 'bench_draw_scores', 'device': torch.cuda.get_device_name(0), 'launch': launch_cost(ops, args.launches, args.repeats, args.warmup)}
    if not args.launch_only:
        out['best_of'] = best_of_cost(args.gen_repeats)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
