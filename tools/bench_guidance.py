"""What classifier-free emotion guidance costs (emo_grammar_step, kind ACC: guide_cond / guide_uncond / guide_scale).
(1) The launch: kind ACC at 32 rows and V = 327 (the rig of bench_sampling_controls.py: randn x 3 logits, every stream drawing in every
    launch) in three cases:
      (a) null    the three fields NULL;
      (b) guided  16 pairs (r, r + 16), scale 1.5: every row reads two logits rows;
      (c) parent  the library of the parent commit (--parent-lib PATH: a libemo_hip.so built from the commit before this feature, driven
                  through a ctypes mirror of ITS block, the one without the three fields) on the launch of (a).  Left out without the flag.
    The cases alternate a, c, b in every repeat; a figure is the median over the repeats of the mean launch time of a back-to-back batch, its
    spread the min / max over the repeats.
(2) End to end, at the shape of bench_stage2_gen.py (d 512, 12 layers, V = 327, bf16, Performer and GPT-2): 16 guided pieces (32 rows of the
    batch) against 32 unguided pieces, AccompanimentLoop.run() with hipGraph replays: accepted tokens per second PER PIECE (a follower's
    tokens are its leader's: they are not counted), and the replayed step.
Writes profiles/guidance_bench.json and prints it as one JSON line.  One run; no pass / fail threshold."""
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
import bench_stage2_gen as s2  # noqa: E402

N, ACC = 32, 1
GUIDE = ('guide_cond', 'guide_uncond', 'guide_scale')
SCALE = 1.5


def pairs():
    half = N // 2
    cond = torch.tensor([r % half for r in range(N)], dtype=torch.int32, device='cuda')
    return dict(guide_cond=cond, guide_uncond=cond + half, guide_scale=torch.full((N,), SCALE, dtype=torch.float32, device='cuda'))


def time_case(ops, case, launches, warmup, parent):
    num, t = bsc.rig(ACC, launches + warmup)
    if case == 'parent':
        args = parent.block(ACC, num, t)
        step = lambda: parent.step(args)                         # noqa: E731
    else:
        held = {}
        args = ops.GrammarStep(kind=ACC)
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
    rec = {'V': 327, 'rows': N, 'pairs': half, 'scale': SCALE}
    for c in cases:
        rec['us_' + c] = round(statistics.median(us[c]), 2)
        rec['us_%s_min_max' % c] = [round(min(us[c]), 2), round(max(us[c]), 2)]
    rec['us_guided_minus_null'] = round(rec['us_guided'] - rec['us_null'], 2)
    if parent:
        rec['us_null_minus_parent'] = round(rec['us_null'] - rec['us_parent'], 2)
        rec['us_spread_null'] = round(max(us['null']) - min(us['null']), 2)
        rec['us_spread_parent'] = round(max(us['parent']) - min(us['parent']), 2)
    return rec


def end_to_end(inf, gl, kind, bars):
    e2i, i2e = s2.vocab()
    m = s2.model(kind, e2i)
    leads, primers = s2.batch(e2i, N, bars)
    out = {}
    for name, pieces in (('unguided', N), ('guided', N // 2)):
        ld, pr, guide = leads[:pieces], primers[:pieces], None
        if name == 'guided':                                     # no Emotion_None in the synthetic vocabulary: Emotion_Q4 stands in
            plan = inf.guidance_plan('bench', SCALE, e2i['Emotion_Q4'], e2i, i2e, pr)
            ld, pr = plan.rows(ld, pr)
            guide = gl.draw_controls('bench', pieces, s2.V, None, s2.TEMP, s2.TOP_P).with_guidance(plan.scales).guide_arg
        loop = inf.AccompanimentLoop(m, e2i, i2e, ld, pr, temp=s2.TEMP, top_p=s2.TOP_P, seed=3, guidance=guide)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(use_graph=True)
        sec = time.perf_counter() - t0
        acc = int(loop.state[:pieces, inf.ACC_S_ACCEPTED].sum().item())
        rs, rsec = loop.replayed
        out[name] = dict(pieces=pieces, rows=loop.n, steps=loop.steps(), accepted_tokens=acc, seconds=round(sec, 4),
                         tokens_per_s_per_piece=round(acc / sec / pieces, 1), replay_ms_per_step=round(1e3 * rsec / max(rs, 1), 4),
                         persistent=loop.eng.persist is not None, **loop.counts())
    out['per_piece_unguided_over_guided'] = round(out['unguided']['tokens_per_s_per_piece'] / out['guided']['tokens_per_s_per_piece'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--bars', type=int, default=8)
    ap.add_argument('--kinds', default='performer,gpt2')
    ap.add_argument('--parent-lib', default=None, help='libemo_hip.so of the commit before the guidance fields: case (c)')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'guidance_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import gen_loop as gl, inference as inf, ops
    torch.cuda.set_device(0)
    bsc.NEW = GUIDE                                              # (ParentLib: the mirror of the parent's block is the current one without these)
    parent = bsc.ParentLib(args.parent_lib) if args.parent_lib else None
    out = {'tool': 'bench_guidance', 'device': torch.cuda.get_device_name(0), 'launches': args.launches, 'repeats': args.repeats, 'runs': 1,
           'parent_lib': bool(parent), 'launch': {'acc': launch_bench(ops, args, parent)}, 'end_to_end': {}}
    with torch.no_grad():
        for kind in [k for k in args.kinds.split(',') if k]:
            out['end_to_end'][kind] = end_to_end(inf, gl, kind, args.bars)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
