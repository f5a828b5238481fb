"""What classifier-free valence guidance costs in stage 1 (emo_grammar_step, kind TXL: guide_cond / guide_uncond / guide_scale).
(1) The launch: kind TXL at 32 rows and V = 200 (the rig of bench_sampling_controls.py: randn x 3 logits, every stream drawing in every
    launch) in three cases:
      (a) null    the three fields NULL;
      (b) guided  16 pairs (r, r + 16), scale 1.5: every row reads two logits rows;
      (c) parent  the library of the parent commit (--parent-lib PATH: a libemo_hip.so built from the commit before this feature; its block is
                  the current one, the fields were there for kind ACC) on the launch of (a).  Left out without the flag.
    The cases alternate a, c, b in every repeat; a figure is the median over the repeats of the mean launch time of a back-to-back batch, its
    spread the min / max over the repeats.  Every difference is reported beside the spreads of its two sides.
(2) End to end, at the shape of bench_stage1_gen.py (d 512, 12 layers, V = 200, bf16), under both model steps: 16 guided pieces (32 rows of the
    batch) against 32 plain pieces, LeadSheetLoop.run() with hipGraph replays: accepted tokens per second PER PIECE and PER BATCH (a follower's
    tokens are its leader's: they are not counted), and the step time.  The vocabulary of bench_stage1_gen.py has no Emotion_None:
    Emotion_Q3 stands in.
Writes profiles/stage1_guidance_bench.json and prints it as one JSON line.  One run; no pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402

import bench_sampling_controls as bsc  # noqa: E402
import bench_stage1_gen as g1  # noqa: E402

N, TXL = 32, 0
SCALE = 1.5
UNCOND = 'Emotion_Q3'


def pairs():
    half = N // 2
    cond = torch.tensor([r % half for r in range(N)], dtype=torch.int32, device='cuda')
    return dict(guide_cond=cond, guide_uncond=cond + half, guide_scale=torch.full((N,), SCALE, dtype=torch.float32, device='cuda'))


def time_case(ops, case, launches, warmup, parent):
    num, t = bsc.rig(TXL, launches + warmup)
    if case == 'parent':
        args = parent.block(TXL, num, t)
        step = lambda: parent.step(args)                         # noqa: E731
    else:
        held = {}
        args = ops.GrammarStep(kind=TXL)
        ops.block_set(args, held, **num, **t)
        if case == 'guided':
            ops.block_set(args, held, **pairs())
        step = lambda: ops.grammar_step(args)                    # noqa: E731
    for _ in range(warmup):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        step()
    b.record()
    torch.cuda.synchronize()
    assert int(t['running'].item()) == N, 'a stream left RUNNING: the launches timed are not all drawing launches'
    return 1e3 * a.elapsed_time(b) / launches, t['seq'].clone()


def launch_bench(ops, args, parent):
    cases = ['null'] + (['parent'] if parent else []) + ['guided']
    us, seqs = {c: [] for c in cases}, {}
    for _ in range(args.repeats):
        for c in cases:
            x, seqs[c] = time_case(ops, c, args.launches, args.warmup, parent)
            us[c].append(x)
    if parent:                                                   # the same draws from the same start: the launch of (a) is the parent's
        assert torch.equal(seqs['null'], seqs['parent'])
    half = N // 2
    assert torch.equal(seqs['guided'][:half], seqs['guided'][half:])          # every follower stayed with its leader
    rec = {'V': 200, 'rows': N, 'pairs': half, 'scale': SCALE}
    for c in cases:
        rec['us_' + c] = round(statistics.median(us[c]), 2)
        rec['us_%s_min_max' % c] = [round(min(us[c]), 2), round(max(us[c]), 2)]
        rec['us_spread_' + c] = round(max(us[c]) - min(us[c]), 2)
    rec['us_guided_minus_null'] = round(rec['us_guided'] - rec['us_null'], 2)
    if parent:
        rec['us_null_minus_parent'] = round(rec['us_null'] - rec['us_parent'], 2)
    return rec


def end_to_end(s1, gl, m, e2i, i2e, step, events):
    emos = ['Q1', 'Q2', 'Q4', 'Positive', 'Negative']
    kw = dict(max_bars=128, max_events=events, temp=1.2, top_p=0.97, representation='functional', key_determine=None, step=step)
    out = {}
    for name, pieces in (('plain', N), ('guided', N // 2)):
        primers, guide = [['Emotion_%s' % emos[i % 5]] for i in range(pieces)], None
        if name == 'guided':
            primers = primers + [[UNCOND]] * pieces
            guide = gl.draw_controls('bench', pieces, g1.V, None, 1.2, 0.97).with_guidance([SCALE] * pieces).guide_arg
        s1.LeadSheetLoop(m, e2i, i2e, primers, seed=99, guidance=guide, **dict(kw, max_events=32)).run(use_graph=True)      # warm-up (kernels, workspaces)
        loop = s1.LeadSheetLoop(m, e2i, i2e, primers, seed=1, guidance=guide, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(use_graph=True)
        sec = time.perf_counter() - t0
        st = loop.state.cpu().numpy()
        if guide is not None:
            assert (st[:pieces] == st[pieces:]).all(), 'a follower left its leader'
        acc = int((st[:pieces, s1.S_LEN] - 1).sum())             # (one-token primers)
        steps = loop.pos - loop.L0
        out[name] = dict(pieces=pieces, rows=loop.n, steps=steps, accepted_tokens=acc, seconds=round(sec, 4), ms_per_step=round(1e3 * sec / max(steps, 1), 4),
                         tokens_per_s_per_piece=round(acc / sec / pieces, 1), tokens_per_s_per_batch=round(acc / sec, 1),
                         finished=int((st[:pieces, s1.S_STATUS] == s1.DONE).sum()))
        del loop
    out['per_piece_plain_over_guided'] = round(out['plain']['tokens_per_s_per_piece'] / out['guided']['tokens_per_s_per_piece'], 3)
    out['per_batch_plain_over_guided'] = round(out['plain']['tokens_per_s_per_batch'] / out['guided']['tokens_per_s_per_batch'], 3)
    out['ms_per_step_guided_minus_plain'] = round(out['guided']['ms_per_step'] - out['plain']['ms_per_step'], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--events', type=int, default=256)
    ap.add_argument('--steps', default='chain,one_launch')
    ap.add_argument('--parent-lib', default=None, help='libemo_hip.so of the commit before this feature: case (c)')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'stage1_guidance_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import gen_loop as gl, ops, stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    torch.cuda.set_device(0)
    bsc.NEW = ()                                                 # (ParentLib: the parent's block is the current one)
    parent = bsc.ParentLib(args.parent_lib) if args.parent_lib else None
    out = {'tool': 'bench_stage1_guidance', 'device': torch.cuda.get_device_name(0), 'launches': args.launches, 'repeats': args.repeats, 'runs': 1,
           'parent_lib': bool(parent), 'launch': {'txl': launch_bench(ops, args, parent)}, 'end_to_end': {}}
    torch.manual_seed(0)
    m = PlainTransformer(g1.D, g1.V, g1.L, g1.H, g1.D, g1.DFF, g1.TGT, g1.TGT, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16').cuda().eval()
    e2i, i2e = g1.vocab()
    out['end_to_end']['shape'] = dict(d_model=g1.D, n_layer=g1.L, V=g1.V, dtype='bf16', max_events=args.events, uncond=UNCOND)
    with torch.no_grad():
        for step in [s for s in args.steps.split(',') if s]:
            out['end_to_end'][step] = end_to_end(s1, gl, m, e2i, i2e, step, args.events)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
