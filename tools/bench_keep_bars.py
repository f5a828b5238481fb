"""What kept bars cost (emo_grammar_step, kinds ACC / ACC_QUEUE: keep_tok / keep_beg / keep_end / n_keep / keep_eos).
(1) The launch: kind ACC at 32 rows and V = 327 (the rig of bench_sampling_controls.py: randn x 3 logits, every stream drawing in every
    launch) in three cases:
      (a) null    the fields NULL: the kernel instance of before;
      (b) keep    the three tables present (every bar of the rig marked drawn: the launch runs the instance that can chain, the draws are
                  the same);
      (c) parent  the library of the parent commit (--parent-lib PATH: a libemo_hip.so built from the commit before this feature, driven
                  through a ctypes mirror of ITS block, the one without the five fields) on the launch of (a).  Left out without the flag.
    The cases alternate a, c, b in every repeat; a figure is the median over the repeats of the mean launch time of a back-to-back batch, its
    spread the min / max over the repeats.  The block grew by 40 bytes; (a) minus (c) is reported beside the two spreads.
(2) End to end, at the shape of bench_stage2_gen.py (d 512, 12 layers, V = 327, bf16, Performer and GPT-2): 32 pieces of 32 bars are generated,
    then bars 14 .. 17 of every piece are drawn again with the other 28 kept, AccompanimentLoop.run() with hipGraph replays: seconds, steps,
    accepted draws and tokens fed, beside the full generation.
Writes profiles/keep_bars_bench.json and prints it as one JSON line.  One run; no pass / fail threshold."""
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
KEEP = ('keep_tok', 'keep_beg', 'keep_end', 'n_keep', 'keep_eos')
BARS, REROLL = 32, range(14, 18)


def time_case(ops, case, launches, warmup, parent):
    num, t = bsc.rig(ACC, launches + warmup)
    if case == 'parent':
        args = parent.block(ACC, num, t)
        step = lambda: parent.step(args)                         # noqa: E731
    else:
        held = {}
        args = ops.GrammarStep(kind=ACC)
        ops.block_set(args, held, **num, **t)
        if case == 'keep':
            bars = t['lead_off'].numel()
            ops.block_set(args, held, n_keep=0, keep_eos=0, keep_tok=torch.zeros(1, dtype=torch.int64, device='cuda'),
                          keep_beg=torch.full((bars,), -1, dtype=torch.int32, device='cuda'), keep_end=torch.zeros(bars, dtype=torch.int32, device='cuda'))
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
    cases = ['null'] + (['parent'] if parent else []) + ['keep']
    us, seqs = {c: [] for c in cases}, {}
    for _ in range(args.repeats):
        for c in cases:
            x, seqs[c] = time_case(ops, c, args.launches, args.warmup, parent)
            us[c].append(x)
    if parent:                                                   # the same draws from the same start: the launch of (a) is the parent's
        assert torch.equal(seqs['null'], seqs['parent'])
    assert torch.equal(seqs['null'], seqs['keep'])
    rec = {'V': 327, 'rows': N, 'block_bytes_added': 40}
    for c in cases:
        rec['us_' + c] = round(statistics.median(us[c]), 2)
        rec['us_%s_min_max' % c] = [round(min(us[c]), 2), round(max(us[c]), 2)]
    rec['us_keep_minus_null'] = round(rec['us_keep'] - rec['us_null'], 2)
    if parent:
        rec['us_null_minus_parent'] = round(rec['us_null'] - rec['us_parent'], 2)
        rec['us_spread_null'] = round(max(us['null']) - min(us['null']), 2)
        rec['us_spread_parent'] = round(max(us['parent']) - min(us['parent']), 2)
        rec['null_minus_parent_inside_the_spreads'] = abs(rec['us_null_minus_parent']) <= max(rec['us_spread_null'], rec['us_spread_parent'])
    return rec


def timed_run(inf, m, e2i, i2e, leads, primers, keep):
    # (Track_Full banned: no grammar rule keeps a random model from drawing it inside a bar, and such a piece does not parse into bars)
    loop = inf.AccompanimentLoop(m, e2i, i2e, leads, primers, temp=s2.TEMP, top_p=s2.TOP_P, seed=3 if keep is None else 4, keep=keep,
                                 banned=[e2i['Track_Full']])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(use_graph=True)
    sec = time.perf_counter() - t0
    rs, rsec = loop.replayed
    state = loop.state.cpu().numpy()
    rec = dict(rows=loop.n, steps=loop.steps(), accepted_draws=int(state[:, inf.ACC_S_ACCEPTED].sum()),
               tokens_fed=int((state[:, inf.ACC_S_CONSUMED] - loop.L0).sum()), seconds=round(sec, 4),
               replay_ms_per_step=round(1e3 * rsec / max(rs, 1), 4), persistent=loop.eng.persist is not None, **loop.counts())
    return rec, loop.results(e2i, i2e, 10000, False, 3)


def end_to_end(inf, kind):
    e2i, i2e = s2.vocab()
    m = s2.model(kind, e2i)
    leads, primers = s2.batch(e2i, N, BARS)
    out = {}
    out['generate'], pieces = timed_run(inf, m, e2i, i2e, leads, primers, None)
    keep = []
    for ids, lead in zip(pieces, leads):                          # a piece that did not finish keeps what it has
        acc = inf.bars_of(ids, e2i)[2] if isinstance(ids, list) else []
        keep.append([None if j in REROLL or j >= len(acc) else acc[j] for j in range(len(lead))])
    out['bars'], out['rerolled_bars'] = BARS, len(REROLL)
    out['kept_bars_per_piece'] = round(sum(sum(b is not None for b in k) for k in keep) / N, 2)
    out['reroll'], again = timed_run(inf, m, e2i, i2e, leads, primers, keep)
    out['kept_bars_verbatim'] = all(isinstance(ids, list) and all(b is None or j >= len(a) - 1 or a[j] == b for j, b in enumerate(k))
                                    for ids, k in zip(again, keep) for a in [inf.bars_of(ids, e2i)[2] if isinstance(ids, list) else []])
    out['reroll_over_generate_seconds'] = round(out['reroll']['seconds'] / out['generate']['seconds'], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--kinds', default='performer,gpt2')
    ap.add_argument('--parent-lib', default=None, help='libemo_hip.so of the commit before the keep fields: case (c)')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'keep_bars_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import inference as inf, ops
    torch.cuda.set_device(0)
    bsc.NEW = KEEP                                               # (ParentLib: the mirror of the parent's block is the current one without these)
    parent = bsc.ParentLib(args.parent_lib) if args.parent_lib else None
    out = {'tool': 'bench_keep_bars', 'device': torch.cuda.get_device_name(0), 'launches': args.launches, 'repeats': args.repeats, 'runs': 1,
           'parent_lib': bool(parent), 'launch': {'acc': launch_bench(ops, args, parent)}, 'end_to_end': {}}
    with torch.no_grad():
        for kind in [k for k in args.kinds.split(',') if k]:
            out['end_to_end'][kind] = end_to_end(inf, kind)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
