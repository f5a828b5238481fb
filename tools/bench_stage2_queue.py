"""Stage-2 generation from a queue against lock-step batches, at the benchmark shape (d512 / L12 / H8, V = 327, bf16, one-launch step), Performer
and GPT-2: 128 synthetic lead sheets of 4 .. 32 bars (spread evenly, in a fixed shuffled order) through 32 rows, two ways in the same process,
alternating twice:
  queue     AccompanimentQueue(slots=32): a row whose job ends takes the next job inside the grammar launch (emo_grammar_step, kind ACC_QUEUE);
  lockstep  four successive runs of 32, jobs in the same order: each is the body of one generate_accompaniments call (AccompanimentLoop built
            and run; the loop object is kept because its step count and replay time are reported; neither way reads its results back inside
            the timed region).
Reported per way and alternation: seconds end to end (tables, engine, prefill and graph capture included), accepted tokens/s, model steps, ms per
step of the replay phase, and for the queue the launches, the slot occupancy and the step ratio queue_plan predicts from the per-job step counts.
Then three launches alone, timed as tools/bench_stage1_queue.py times launches: kind ACC_QUEUE against kind ACC at 32 rows that all draw, and
emo_favor_state_reset at the Performer's shape with no row flagged and with 4 flagged.  Writes profiles/stage2_queue_bench.json and prints it as
one JSON line.  No pass / fail threshold."""
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

SLOTS, JOBS, V, L, H, D, DFF, NF = 32, 128, 327, 12, 8, 512, 2048, 128


def vocab():
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4')] + ['Key_%s' % k for k in ('C', 'a', 'G', 'e')] + ['Tempo_110']
             + ['Track_LeadSheet', 'Track_Full', 'Bar_None'] + ['Beat_%d' % i for i in range(16)] + ['Chord_%d_M' % i for i in range(40)])
    names += ['Note_Pitch_%d' % i for i in range(V - 2 - len(names))] + ['EOS_None', 'PAD_None']
    return {e: i for i, e in enumerate(names)}, dict(enumerate(names))


def model(kind, e2i):
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    torch.manual_seed(3)
    if kind == 'performer':
        m = MusicPerformer(V, L, H, D, DFF, D, favor_feature_dims=NF, use_segment_emb=True, n_segment_types=2, compute_dtype='bf16', redraw='fixed')
    else:
        m = MusicGPT2(V, L, H, D, DFF, D, use_segment_emb=True, n_segment_types=2, dropout=0.1, compute_dtype='bf16')
    with torch.no_grad():                          # bars end after ~15 events, Beats are common, pieces finish
        b = m.dec_out_proj.bias
        b[e2i['Track_LeadSheet']] += 4.0
        for k in range(16):
            b[e2i['Beat_%d' % k]] += 2.0
    return m.cuda().eval()


def jobs(e2i):
    rs = np.random.RandomState(1)
    pool = [e2i['Beat_%d' % k] for k in range(16)] + [e2i['Chord_%d_M' % k] for k in range(40)]
    order = [(i * 37) % JOBS for i in range(JOBS)]                    # 37 and 128 are coprime: every length once, long and short mixed
    bars = [4 + (28 * k) // (JOBS - 1) for k in order]
    leads = [[[e2i['Bar_None']] + sorted(rs.choice(pool, size=rs.randint(2, 7)).tolist()) for _ in range(nb)] for nb in bars]
    primers = [[e2i['Emotion_Q%d' % (1 + i % 4)], e2i[['Key_C', 'Key_a'][i % 2]], e2i['Tempo_110']] for i in range(JOBS)]
    return leads, primers, bars


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def run_queue(inf, s1, m, e2i, i2e, leads, primers, kw):
    def go():
        q = inf.AccompanimentQueue(m, e2i, i2e, leads, primers, SLOTS, **kw)
        q.run()
        return q
    q, sec = timed(go)
    assert q.eng.persist is not None, 'the one-launch step does not run here'
    steps = q.job_steps()
    launches, occ = s1.queue_plan(steps, SLOTS)
    lock = sum(max(steps[i:i + SLOTS]) for i in range(0, JOBS, SLOTS))
    acc = q.accepted_tokens()
    return dict(seconds=sec, accepted=acc, tokens_per_s=acc / sec, launches=q.launches, launches_planned=launches, occupancy=occ,
                replayed_steps=q.replayed[0], ms_per_step=1e3 * q.replayed[1] / max(1, q.replayed[0]),
                lockstep_steps_planned=lock, step_ratio_planned=lock / float(launches), counts=q.counts())


def run_lockstep(inf, s1, m, e2i, i2e, leads, primers, kw):
    def go():
        loops = []
        for i in range(0, JOBS, SLOTS):
            loop = inf.AccompanimentLoop(m, e2i, i2e, leads[i:i + SLOTS], primers[i:i + SLOTS], **dict(kw, seed=kw['seed'] + i // SLOTS))
            loop.run()
            loops.append(loop)
        return loops
    loops, sec = timed(go)
    rs, rt = sum(lp.replayed[0] for lp in loops), sum(lp.replayed[1] for lp in loops)
    acc = sum(lp.accepted_tokens() for lp in loops)
    counts = {k: sum(lp.counts()[k] for lp in loops) for k in loops[0].counts()}
    return dict(seconds=sec, accepted=acc, tokens_per_s=acc / sec, steps=sum(lp.steps() for lp in loops), replayed_steps=rs,
                ms_per_step=1e3 * rt / max(1, rs), counts=counts)


def grammar_rig(ops, kind, launches):
    """32 rows that draw plain events in every launch; the queue kind with every slot holding a running job."""
    N, dev = SLOTS, 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    flags = torch.zeros(V, dtype=torch.int32, device=dev)
    flags[V - 1] = 4                                                  # PAD
    width = launches + 16
    params, state = torch.zeros(N, 8, dtype=torch.int32, device=dev), torch.zeros(N, 8, dtype=torch.int32, device=dev)
    params[:, 0], params[:, 1], params[:, 4] = 1 << 20, 1 << 20, 1
    state[:, 1], state[:, 2] = 3, 3                                   # LEN = CONSUMED = 3: every launch draws
    t = dict(logits=(torch.randn(N, V, device=dev, generator=g) * 3).contiguous(), u_steps=torch.rand(4 * launches, N, device=dev, generator=g),
             ev_flags=flags, ev_beat=torch.zeros(V, dtype=torch.int32, device=dev), params=params, state=state,
             seq=torch.zeros(N, width, dtype=torch.int64, device=dev), segs=torch.zeros(N, width, dtype=torch.int64, device=dev),
             lead_tok=torch.zeros(4, dtype=torch.int64, device=dev), lead_off=torch.zeros(N + 1, dtype=torch.int32, device=dev),
             running=torch.tensor([N], dtype=torch.int32, device=dev), tok_out=torch.zeros(N, dtype=torch.int64, device=dev),
             seg_out=torch.zeros(N, dtype=torch.int64, device=dev))
    t['logits'][:, V - 12] = -60.0                                    # (Track_LeadSheet out of reach: only plain events)
    num = dict(n_rows=N, n_token=V, ld_u=N, temperature=1.2, top_p=0.9, max_len=1 << 20, track_full=10, pad=V - 1)
    if kind == ops.GRAMMAR_ACC_QUEUE:
        num.update(n_jobs=N, mem_rows=1 << 30)
        t.update(slot_job=torch.arange(N, dtype=torch.int32, device=dev), queue_head=torch.tensor([N], dtype=torch.int32, device=dev),
                 mem_lens=torch.zeros(N, dtype=torch.int64, device=dev), job_steps=torch.zeros(N, dtype=torch.int32, device=dev),
                 row_reset=torch.zeros(N, dtype=torch.int32, device=dev))
    args, held = ops.GrammarStep(kind=kind), {}
    ops.block_set(args, held, **num, **t)
    return args, held, t


def time_calls(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / launches


def launch_cost(ops, launches, repeats, warmup):
    out = {'rows': SLOTS, 'V': V, 'launches': launches, 'repeats': repeats}
    acc, queue = [], []
    for _ in range(repeats):
        for kind, sink in ((ops.GRAMMAR_ACC, acc), (ops.GRAMMAR_ACC_QUEUE, queue)):
            args, held, t = grammar_rig(ops, kind, launches + warmup)
            sink.append(time_calls(lambda: ops.grammar_step(args), launches, warmup))
            assert int(t['running'].item()) == SLOTS, 'a row left RUNNING: the launches timed are not all drawing launches'
    out.update(us_acc=round(statistics.median(acc), 2), us_acc_queue=round(statistics.median(queue), 2),
               us_acc_min_max=[round(min(acc), 2), round(max(acc), 2)], us_acc_queue_min_max=[round(min(queue), 2), round(max(queue), 2)])
    S = [torch.ones(SLOTS, H, NF, D // H, device='cuda') for _ in range(L)]
    z = [torch.ones(SLOTS, H, NF, device='cuda') for _ in range(L)]
    table = torch.tensor([[S[l].data_ptr(), z[l].data_ptr()] for l in range(L)], dtype=torch.int64, device='cuda')
    for name, rows in (('us_reset_none_flagged', []), ('us_reset_4_flagged', [3, 9, 17, 30])):
        flags = torch.zeros(SLOTS, dtype=torch.int32, device='cuda')
        flags[rows] = 1
        us = [time_calls(lambda: ops.favor_state_reset(table, SLOTS, H * NF * (D // H), H * NF, flags), launches, warmup) for _ in range(repeats)]
        out[name] = round(statistics.median(us), 2)
        out[name + '_min_max'] = [round(min(us), 2), round(max(us), 2)]
    out['reset_bytes_per_row'] = 4 * L * (H * NF * (D // H) + H * NF)
    return out


def rounded(r):
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--alternations', type=int, default=2)
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--launch-repeats', type=int, default=7)
    ap.add_argument('--kinds', default='performer,gpt2')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'stage2_queue_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import inference as inf, ops, stage1_inference as s1
    torch.cuda.set_device(0)
    e2i, i2e = vocab()
    leads, primers, bars = jobs(e2i)
    kw = dict(max_events=10000, temp=1.2, top_p=0.9, seed=1)
    out = {'tool': 'bench_stage2_queue', 'device': torch.cuda.get_device_name(0), 'slots': SLOTS, 'jobs': JOBS, 'bars': [min(bars), max(bars)],
           'note': 'one run on one machine'}
    for kind in args.kinds.split(','):
        m = model(kind, e2i)
        run_queue(inf, s1, m, e2i, i2e, leads, primers, kw)                          # warm-up of both ways
        run_lockstep(inf, s1, m, e2i, i2e, leads, primers, kw)
        rec = {'queue': [], 'lockstep': []}
        for _ in range(args.alternations):
            rec['queue'].append(rounded(run_queue(inf, s1, m, e2i, i2e, leads, primers, kw)))
            rec['lockstep'].append(rounded(run_lockstep(inf, s1, m, e2i, i2e, leads, primers, kw)))
        qs, ls = rec['queue'], rec['lockstep']
        rec['tokens_per_s'] = {'queue': [r['tokens_per_s'] for r in qs], 'lockstep': [r['tokens_per_s'] for r in ls]}
        rec['ms_per_step'] = {'queue': [r['ms_per_step'] for r in qs], 'lockstep': [r['ms_per_step'] for r in ls]}
        rec['step_ratio_measured'] = round(ls[0]['steps'] / float(qs[0]['launches']), 4)
        rec['step_ratio_planned'] = qs[0]['step_ratio_planned']
        rec['speedup_end_to_end'] = [round(a['seconds'] / b['seconds'], 4) for a, b in zip(ls, qs)]
        out[kind] = rec
        del m
    out['launch'] = launch_cost(ops, args.launches, args.launch_repeats, 20)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
