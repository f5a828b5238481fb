"""What kept bars cost in stage 1 (emo_grammar_step, kinds TXL and TXL_QUEUE: keep_tok / keep_beg / keep_end / n_keep / keep_bar / keep_left).
(1) The launches: kind TXL at 32 rows and V = 200 (the rig of bench_sampling_controls.py: randn x 3 logits, every stream drawing in every
    launch) and kind TXL_QUEUE on the same rig as 32 jobs in 32 slots (the warm-up launches admit the jobs and feed their primers), each in
    three cases:
      (a) null    the new fields NULL;
      (b) keep    the tables present (four kept-bar entries per stream, two of them kept): the <.., true> instance on its drawing path;
      (c) parent  the library of the parent commit (--parent-lib PATH: a libemo_hip.so built from the commit before this feature, driven through
                  a ctypes mirror of ITS block, the one without keep_bar / keep_left) on the launch of (a).  Left out without the flag.
    The cases alternate a, c, b in every repeat; a figure is the median over the repeats of the mean launch time of a back-to-back batch, its
    spread the min / max over the repeats.  From the same start and the same draws the launch of (a) must leave the parent's state and rows,
    word for word: asserted.
(2) End to end, at the shape of bench_stage1_gen.py (d 512, 12 layers, V = 200, bf16; the output bias of Bar_None raised so that a bar is a
    handful of tokens), under both model steps: 32 pieces of 32 bars generated whole, then bars 14 .. 17 of each drawn again with the other 28
    kept (generate_lead_sheets' own path: LeadSheetLoop.run() with hipGraph replays): steps, seconds and the ratio.  A kept token still costs a
    model step; what a re-roll saves is the rejected draws inside the kept bars.
(3) bench.py is run beside this tool, not by it.
Writes profiles/stage1_keep_bars_bench.json and prints it as one JSON line.  One run; no pass / fail threshold."""
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

N, TXL, TXL_QUEUE = 32, 0, 3
BARS, REROLL = 32, (14, 18)


def rig(kind, launches):
    num, t = bsc.rig(TXL, launches)
    if kind == TXL_QUEUE:
        t['logits'][:] = t['logits'][0].clone()                  # (which slot admits which job is not specified: every slot shows the same row)
        num.update(n_jobs=N, mem_rows=1 << 20)
        t.update(slot_job=torch.full((N,), -1, dtype=torch.int32, device='cuda'), queue_head=torch.zeros(1, dtype=torch.int32, device='cuda'),
                 mem_lens=torch.zeros(N, dtype=torch.int64, device='cuda'))
    return num, t


def keep_tables(params):
    """Four entries per stream, bars 1 and 2 kept (two tokens each); no stream ever draws a Bar, so every launch stays a drawing launch."""
    beg, end = [], []
    for r in range(N):
        params[r, 6], params[r, 7] = 4 * r, 4
        beg += [-1, 4 * r, 4 * r + 2, -1]
        end += [0, 4 * r + 2, 4 * r + 4, 0]
    dev = 'cuda'
    return dict(n_keep=4 * N, keep_bar=5, keep_tok=torch.full((4 * N,), 7, dtype=torch.int64, device=dev),
                keep_beg=torch.tensor(beg, dtype=torch.int32, device=dev), keep_end=torch.tensor(end, dtype=torch.int32, device=dev),
                keep_left=torch.zeros(N, dtype=torch.int32, device=dev))


def time_case(ops, kind, case, launches, warmup, parent):
    num, t = rig(kind, launches + warmup)
    if case == 'parent':
        args = parent.block(kind, num, t)
        step = lambda: parent.step(args)                         # noqa: E731
    else:
        held = {}
        args = ops.GrammarStep(kind=kind)
        more = keep_tables(t['params']) if case == 'keep' else {}
        ops.block_set(args, held, **num, **t, **more)
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
    draws = t['state'][:, 7].clone()
    assert int(draws.min().item()) >= launches, 'a launch that was timed did not draw'
    return 1e3 * a.elapsed_time(b) / launches, (t['state'].clone(), t['seq'].clone())


def launch_bench(ops, kind, args, parent):
    cases = ['null'] + (['parent'] if parent else []) + ['keep']
    us, left = {c: [] for c in cases}, {}
    for _ in range(args.repeats):
        for c in cases:
            x, left[c] = time_case(ops, kind, c, args.launches, args.warmup, parent)
            us[c].append(x)
    if parent:                                                   # the same draws from the same start: the launch of (a) is the parent's, word for word
        assert torch.equal(left['null'][0], left['parent'][0]) and torch.equal(left['null'][1], left['parent'][1])
    assert torch.equal(left['null'][1], left['keep'][1])         # (no Bar is drawn: the tables change nothing but the instance)
    rec = {'V': 200, 'rows': N}
    for c in cases:
        rec['us_' + c] = round(statistics.median(us[c]), 2)
        rec['us_%s_min_max' % c] = [round(min(us[c]), 2), round(max(us[c]), 2)]
        rec['us_spread_' + c] = round(max(us[c]) - min(us[c]), 2)
    rec['us_keep_minus_null'] = round(rec['us_keep'] - rec['us_null'], 2)
    if parent:
        rec['us_null_minus_parent'] = round(rec['us_null'] - rec['us_parent'], 2)
        rec['null_equals_parent_word_for_word'] = True
    return rec


def timed_run(s1, m, e2i, i2e, primers, **kw):
    s1.LeadSheetLoop(m, e2i, i2e, primers, seed=99, **dict(kw, max_events=min(48, kw['max_events']))).run(use_graph=True)     # warm-up (kernels, workspaces)
    loop = s1.LeadSheetLoop(m, e2i, i2e, primers, seed=1, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(use_graph=True)
    sec = time.perf_counter() - t0
    st = loop.state.cpu().numpy()
    rec = dict(steps=loop.pos - loop.L0, seconds=round(sec, 4), ms_per_step=round(1e3 * sec / max(loop.pos - loop.L0, 1), 4),
               draws=int(st[:, s1.S_DRAWS].sum()), tokens=int(st[:, s1.S_LEN].sum()), finished=int((st[:, s1.S_STATUS] == s1.DONE).sum()))
    return rec, loop.results()


def split(s1, ids, e2i):
    """bars_of, or ([], [], False) for a result that is no id list or holds no Bar."""
    if not isinstance(ids, list) or e2i['Bar_None'] not in ids:
        return [], [], False
    return s1.bars_of(ids, e2i)


def end_to_end(s1, m, e2i, i2e, step, events):
    emos = ['Q1', 'Q2', 'Q4', 'Positive', 'Negative']
    # (EOS_None is banned: an EOS drawn inside a bar ends the piece there, whole or re-rolled, and the comparison is about pieces of 32 bars)
    kw = dict(max_events=events, temp=1.2, top_p=0.97, representation='functional', key_determine=None, step=step, banned=[e2i['EOS_None']])
    whole, res = timed_run(s1, m, e2i, i2e, [['Emotion_%s' % emos[i % 5]] for i in range(N)], max_bars=BARS + 1, **kw)
    primers, keep, max_bars, left_out = [], [], [], 0
    for ids in res:
        head, bars, _ = split(s1, ids, e2i)
        if len(bars) != BARS:                                    # (a piece that ended on max_events: it takes no part, a stand-in keeps the batch at 32 rows)
            left_out += 1
            continue
        primers.append([i2e[t] for t in head])
        keep.append([None if REROLL[0] <= j < REROLL[1] else bars[j] for j in range(BARS)])
        max_bars.append(BARS + 1)
    assert primers, 'no piece of %d bars: raise --events' % BARS
    while len(primers) < N:
        primers.append(primers[0]), keep.append(keep[0]), max_bars.append(max_bars[0])
    again, res2 = timed_run(s1, m, e2i, i2e, primers, max_bars=max_bars, keep=keep, **kw)
    same = 0
    for ids, kept in zip(res2, keep):
        bars = split(s1, ids, e2i)[1]
        same += int(len(bars) == BARS and all(bars[j] == kept[j] for j in range(BARS) if kept[j] is not None))
    again['pieces_with_every_kept_bar_as_given'] = same
    return dict(whole=whole, reroll=again, bars=BARS, rerolled_bars=list(REROLL), pieces_not_of_32_bars=left_out,
                seconds_reroll_over_whole=round(again['seconds'] / whole['seconds'], 3), steps_reroll_over_whole=round(again['steps'] / whole['steps'], 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--events', type=int, default=768)
    ap.add_argument('--steps', default='chain,one_launch')
    ap.add_argument('--bar-bias', type=float, default=4.0, help='added to the output bias of Bar_None: bars of a handful of tokens')
    ap.add_argument('--parent-lib', default=None, help='libemo_hip.so of the commit before this feature: case (c)')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'stage1_keep_bars_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import ops, stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    torch.cuda.set_device(0)
    bsc.NEW = ('keep_bar', 'keep_left')                          # (ParentLib: the parent's block is the current one without the two)
    parent = bsc.ParentLib(args.parent_lib) if args.parent_lib else None
    out = {'tool': 'bench_stage1_keep_bars', 'device': torch.cuda.get_device_name(0), 'launches': args.launches, 'repeats': args.repeats, 'runs': 1,
           'parent_lib': bool(parent), 'launch': {'txl': launch_bench(ops, TXL, args, parent), 'txl_queue': launch_bench(ops, TXL_QUEUE, args, parent)},
           'end_to_end': {}}
    torch.manual_seed(0)
    m = PlainTransformer(g1.D, g1.V, g1.L, g1.H, g1.D, g1.DFF, g1.TGT, g1.TGT, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16')
    e2i, i2e = g1.vocab()
    with torch.no_grad():
        m.dec_out_proj.bias[e2i['Bar_None']] += args.bar_bias
    m = m.cuda().eval()
    out['end_to_end']['shape'] = dict(d_model=g1.D, n_layer=g1.L, V=g1.V, dtype='bf16', max_events=args.events, streams=N, bar_bias=args.bar_bias)
    with torch.no_grad():
        for step in [s for s in args.steps.split(',') if s]:
            out['end_to_end'][step] = end_to_end(s1, m, e2i, i2e, step, args.events)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
