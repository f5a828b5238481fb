#!/usr/bin/env python3
"""Scoring pass at the benchmark shape (64 x 2048 tokens, V = 327, bf16), both stage-2 backbones, in one process:
  (a) eval-mode no_grad forward + compute_loss('mean')   — what validate() does per batch
  (b) scoring.score_tokens with logprob, rank and entropy
alternated, timed with HIP events after a warm-up.  --kernel-only runs emo_token_scores alone on a [M, 512] padded buffer (for a
`rocprofv3 --kernel-trace --stats` run of its own) and reports it against its floor: M x ld x 4 bytes read once at 5.5 TB/s.
Writes one JSON object (--out)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_RATE = 5.5e12        # achievable HBM read rate the project measures against (README)


def _model(kind, dtype):
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    V, L, H, d, dff = 327, 12, 8, 512, 2048
    torch.manual_seed(0)
    if kind == 'performer':
        m = MusicPerformer(V, L, H, d, dff, d, dropout=0.1, favor_feature_dims=128, use_segment_emb=True, n_segment_types=2, compute_dtype=dtype,
                           redraw='fixed')
    else:
        m = MusicGPT2(V, L, H, d, dff, d, dropout=0.1, use_segment_emb=True, n_segment_types=2, compute_dtype=dtype)
    return m.cuda().eval()


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def bench_model(kind, B, T, dtype, warmup, rounds, reps):
    from emo_disentanger_amd import scoring
    from emo_disentanger_amd.data import synthetic_batch
    m = _model(kind, dtype)
    b = synthetic_batch(m.n_token, B, T, seed=1, realistic_targets=True, device='cuda')
    x, seg, tgt = b['dec_input'], b['track_mask'], b['dec_target']

    def a():
        with torch.no_grad():
            return m.compute_loss(m(x, seg_inp=seg), tgt)['recons_loss']

    def s():
        return scoring.score_tokens(m, x, tgt, seg_inp=seg)

    for _ in range(warmup):
        a(), s()
    torch.cuda.synchronize()
    ta, ts = [], []
    for _ in range(rounds):                      # alternate, same process, same box
        ta.append(_time(a, reps))
        ts.append(_time(s, reps))
    ma, ms = sorted(ta)[len(ta) // 2], sorted(ts)[len(ts) // 2]
    return {'model': kind, 'B': B, 'T': T, 'dtype': dtype, 'forward_plus_mean_loss_ms': ma, 'score_tokens_ms': ms, 'ratio': ms / ma,
            'tokens_per_s_scored': B * T / (ms * 1e-3), 'rounds_ms': {'a': ta, 'b': ts}}


def bench_kernel(M, V, ld, warmup, reps):
    from emo_disentanger_amd import ops
    buf = torch.full((M, ld), -1e30, device='cuda')
    buf[:, :V] = torch.randn(M, V, device='cuda') * 3
    tgt = torch.randint(0, V - 1, (M,), device='cuda')
    view = buf[:, :V]
    for _ in range(warmup):
        ops.token_scores(view, tgt, V - 1)
    ms = _time(lambda: ops.token_scores(view, tgt, V - 1), reps)
    floor_ms = M * ld * 4 / HBM_RATE * 1e3
    read_ms = M * V * 4 / HBM_RATE * 1e3
    return {'kernel': 'emo_token_scores', 'M': M, 'V': V, 'ld': ld, 'ms_by_events_incl_launch': ms, 'floor_ms_full_rows': floor_ms,
            'floor_ms_columns_read': read_ms, 'share_of_floor': floor_ms / ms}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--seq', type=int, default=2048)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--models', default='performer,gpt2')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernel-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'bench_scoring needs a GPU'
    res = {'kernel': bench_kernel(args.batch * args.seq, 327, 512, 3, 20)}
    if not args.kernel_only:
        res['models'] = [bench_model(k, args.batch, args.seq, args.dtype, args.warmup, args.rounds, args.reps) for k in args.models.split(',')]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
