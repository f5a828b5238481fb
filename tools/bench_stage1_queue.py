"""Stage-1 generation from a queue against lock-step batches, at the emopia_finetune.yaml shape (d512 / L12 / H8, V = 200, bf16): 128 jobs with
mixed per-job max_events (64 .. 512, spread evenly, in a fixed shuffled order; the synthetic weights all but never draw EOS, so max_events is
what ends a job) through 32 rows, two ways in the same process:
  queue     LeadSheetQueue(slots=32): a row whose job ends takes the next job inside the grammar launch (emo_grammar_step, kind TXL_QUEUE);
  lockstep  four successive runs of 32, jobs in the same order: each is the body of one generate_lead_sheets call (LeadSheetLoop built and run; the
            loop object is kept because its step count and replay time are reported, which the public function does not return; neither
            way reads its results back inside the timed region);
for step='chain' and step='one_launch'.  Reported per way: seconds end to end (tables, memory, prefill and graph capture included), accepted
tokens/s, model steps, ms per step of the replay phase, and for the queue the launches, the slot occupancy and the step ratio queue_plan predicts
from the per-job step counts.  Then the grammar launch alone, kind TXL_QUEUE against kind TXL at 32 rows that all draw, timed as
tools/bench_draw_scores.py times launches.  Writes profiles/stage1_queue_bench.json and prints it as one JSON line.  No pass / fail threshold."""
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

SLOTS, JOBS = 32, 128


def jobs():
    emos = ['Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative']
    order = [(i * 37) % JOBS for i in range(JOBS)]                    # 37 and 128 are coprime: every length once, long and short mixed
    return [['Emotion_%s' % emos[i % 6]] for i in range(JOBS)], [64 + (448 * k) // (JOBS - 1) for k in order]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def run_queue(s1, m, e2i, i2e, primers, max_events, step, kw):
    def go():
        q = s1.LeadSheetQueue(m, e2i, i2e, primers, SLOTS, max_events=max_events, step=step, **kw)
        q.run()
        return q
    q, sec = timed(go)
    steps = q.job_steps()
    launches, occ = s1.queue_plan(steps, SLOTS)
    lock = sum(max(steps[i:i + SLOTS]) for i in range(0, JOBS, SLOTS))
    return dict(seconds=sec, accepted=q.accepted_tokens(), launches=q.launches, launches_planned=launches, occupancy=occ,
                replayed_steps=q.replayed[0], ms_per_step=1e3 * q.replayed[1] / max(1, q.replayed[0]),
                lockstep_steps_planned=lock, step_ratio_planned=lock / float(launches),
                statuses=sorted(set(q.state[:, s1.S_STATUS].cpu().tolist())))


def run_lockstep(s1, m, e2i, i2e, primers, max_events, step, kw):
    def go():
        loops = []
        for i in range(0, JOBS, SLOTS):
            loop = s1.LeadSheetLoop(m, e2i, i2e, primers[i:i + SLOTS], max_events=max_events[i:i + SLOTS], step=step,
                                    **dict(kw, seed=kw['seed'] + i // SLOTS))
            loop.run()
            loops.append(loop)
        return loops
    loops, sec = timed(go)
    rs, rt = sum(lp.replayed[0] for lp in loops), sum(lp.replayed[1] for lp in loops)
    return dict(seconds=sec, accepted=sum(lp.accepted_tokens() for lp in loops), steps=sum(lp.pos - lp.L0 for lp in loops),
                replayed_steps=rs, ms_per_step=1e3 * rt / max(1, rs))


def launch_rig(ops, kind, launches):
    """32 rows that draw in every launch (bench_draw_scores.rig, kind TXL); the queue kind with every slot holding a running job."""
    N, V, dev = SLOTS, 200, 'cuda'
    g = torch.Generator(device=dev).manual_seed(0)
    flags = torch.zeros(V, dtype=torch.int32, device=dev)
    flags[V - 1] = 4
    params, state = torch.zeros(N, 8, dtype=torch.int32, device=dev), torch.zeros(N, 8, dtype=torch.int32, device=dev)
    state[:, 1] = 3
    params[:, 0], params[:, 1], params[:, 2], state[:, 6] = 1 << 20, 1 << 20, 3, 3
    t = dict(logits=(torch.randn(N, V, device=dev, generator=g) * 3).contiguous(), u_steps=torch.rand(4 * launches, N, device=dev, generator=g),
             ev_flags=flags, ev_beat=torch.zeros(V, dtype=torch.int32, device=dev), params=params, state=state,
             seq=torch.zeros(N, launches + 16, dtype=torch.int64, device=dev), running=torch.tensor([N], dtype=torch.int32, device=dev),
             tok_out=torch.zeros(N, dtype=torch.int64, device=dev))
    num = dict(n_rows=N, n_token=V, ld_u=N, temperature=1.2, top_p=0.9, key_temperature=1.1, key_top_p=0.97)
    if kind == ops.GRAMMAR_TXL_QUEUE:
        num.update(n_jobs=N, mem_rows=1 << 30)
        t.update(slot_job=torch.arange(N, dtype=torch.int32, device=dev), queue_head=torch.tensor([N], dtype=torch.int32, device=dev),
                 mem_lens=torch.zeros(N, dtype=torch.int64, device=dev), job_steps=torch.zeros(N, dtype=torch.int32, device=dev))
    args, held = ops.GrammarStep(kind=kind), {}
    ops.block_set(args, held, **num, **t)
    return args, held, t


def time_launches(ops, kind, launches, warmup):
    args, held, t = launch_rig(ops, kind, launches + warmup)
    for _ in range(warmup):
        ops.grammar_step(args)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        ops.grammar_step(args)
    b.record()
    torch.cuda.synchronize()
    assert int(t['running'].item()) == SLOTS, 'a row left RUNNING: the launches timed are not all drawing launches'
    return 1e3 * a.elapsed_time(b) / launches, int(t['state'][:, 2].sum().item())


def launch_cost(ops, launches, repeats, warmup):
    txl, queue = [], []
    for _ in range(repeats):
        us0, acc0 = time_launches(ops, ops.GRAMMAR_TXL, launches, warmup)
        us1, acc1 = time_launches(ops, ops.GRAMMAR_TXL_QUEUE, launches, warmup)
        assert acc0 == acc1                                           # the same draws either way
        txl.append(us0)
        queue.append(us1)
    return dict(rows=SLOTS, V=200, launches=launches, repeats=repeats, us_txl=round(statistics.median(txl), 2),
                us_txl_queue=round(statistics.median(queue), 2), us_txl_min_max=[round(min(txl), 2), round(max(txl), 2)],
                us_txl_queue_min_max=[round(min(queue), 2), round(max(queue), 2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--launch-repeats', type=int, default=7)
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'stage1_queue_bench.json'))
    args = ap.parse_args()
    import bench_stage1_gen as b1
    from emo_disentanger_amd import ops, stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    m = PlainTransformer(b1.D, b1.V, b1.L, b1.H, b1.D, b1.DFF, b1.TGT, b1.TGT, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16',
                         max_gen_len=1024).cuda().eval()
    e2i, i2e = b1.vocab()
    primers, max_events = jobs()
    kw = dict(max_bars=128, temp=1.2, top_p=0.97, representation='functional', key_determine=None, seed=1)
    out = {'tool': 'bench_stage1_queue', 'device': torch.cuda.get_device_name(0), 'slots': SLOTS, 'jobs': JOBS, 'max_events': [min(max_events), max(max_events)],
           'note': 'one run on one machine'}
    for step in s1.STEPS:
        rec = {}
        for name, run in (('queue', run_queue), ('lockstep', run_lockstep)):
            run(s1, m, e2i, i2e, primers, max_events, step, kw)                     # warm-up
            runs = [run(s1, m, e2i, i2e, primers, max_events, step, kw) for _ in range(args.repeats)]
            r = sorted(runs, key=lambda x: x['seconds'])[len(runs) // 2]             # the run of median end-to-end time
            r['seconds_all'] = [round(x['seconds'], 4) for x in runs]
            r['tokens_per_s'] = round(r['accepted'] / r['seconds'], 1)
            rec[name] = {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}
        rec['step_ratio_measured'] = round(rec['lockstep']['steps'] / float(rec['queue']['launches']), 4)
        rec['speedup_end_to_end'] = round(rec['lockstep']['seconds'] / rec['queue']['seconds'], 4)
        out[step] = rec
    out['launch'] = launch_cost(ops, args.launches, args.launch_repeats, 20)
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
