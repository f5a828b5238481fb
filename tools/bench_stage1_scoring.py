"""Stage-1 lead-sheet scoring at the emopia_finetune.yaml shape (d 512, 12 layers, 8 heads, d_ff 2048, V = 200, bf16, mem_len 512, seeded
random weights): 16 pieces x 2048 tokens scored three ways in one process on one device —
  windowed   scoring.score_lead_sheet_tokens: one forward_windowed (banded relative attention, window = mem_len) + one emo_token_scores launch;
  decode     the same pieces through the generator's own path: a 1-token prefill, then one decode_step and one emo_token_scores launch per
             token (what scoring cost before the band existed; eager launches, as a scoring loop over given tokens has no fixed replay unit);
  causal     the unwindowed forward at the same T + one emo_token_scores launch (other numbers past position mem_len: the cost yardstick of
             the band, O(T^2) against O(T mem_len) attention work).
Each is warmed up once, then timed with HIP events over --reps runs (decode: one run).  Also reports the largest log-probability difference
between windowed and decode over the scored positions.  Prints one JSON line and writes it to --out (default
profiles/stage1_scoring_bench.json).  Arguments: --pieces N (16), --tokens T (2048), --reps R (5), --out PATH."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

D, L, H, DFF, V, MEM = 512, 12, 8, 2048, 200, 512


def timed(fn, reps):
    """Median milliseconds of fn() over `reps` runs, each between two HIP events on the current stream."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2], ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pieces', type=int, default=16)
    ap.add_argument('--tokens', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stage1_scoring_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import ops, scoring
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    n, T = args.pieces, args.tokens
    m = PlainTransformer(D, V, L, H, D, DFF, MEM, MEM, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16', max_gen_len=T).cuda().eval()
    pad = V - 1
    tok = torch.randint(0, pad, (n, T), generator=torch.Generator().manual_seed(1)).cuda()
    lengths, primer = [T] * n, 1
    tgt = scoring.lead_sheet_targets(tok, lengths, primer, pad)
    out = {'tool': 'bench_stage1_scoring', 'shape': dict(d_model=D, n_layer=L, n_head=H, d_ff=DFF, V=V, mem_len=MEM, dtype='bf16'), 'pieces': n,
           'tokens': T, 'scored_tokens': int((tgt != pad).sum()), 'reps': args.reps}

    res = {}

    def windowed():
        res['w'] = scoring.score_lead_sheet_tokens(m, tok, lengths, primer)
    windowed()
    out['windowed_ms'], out['windowed_ms_runs'] = timed(windowed, args.reps)

    x = tok.t().contiguous()

    def decode(steps=T):
        lp = torch.zeros(n, steps, device=tok.device)
        _, mem = m.generate(x[:1], tuple())                           # (it returns stream 0's logits only: position 0 is scored from a prefill of its own)
        h, _, _ = m._prefill(x[:1])
        lp[:, 0] = -ops.token_scores(m._logits(h), tgt[:, 0].contiguous(), pad, want=())['nll']
        for i in range(1, steps):
            lp[:, i] = -ops.token_scores(m.decode_step(x[i], mem), tgt[:, i].contiguous(), pad, want=())['nll']
        res['d'] = lp
    with torch.no_grad():
        decode(8)
        out['decode_ms'], _ = timed(decode, 1)

    def causal():
        with torch.no_grad():
            h, _, _ = m._prefill(x)
            res['c'] = ops.token_scores(m._logits(h), tgt.reshape(-1), pad, want=('rank', 'entropy'))
    causal()
    out['causal_ms'], out['causal_ms_runs'] = timed(causal, args.reps)

    mask = tgt != pad
    out['max_logprob_diff_windowed_vs_decode'] = float((res['w'].logprob - res['d'])[mask].abs().max())
    out['decode_over_windowed'] = round(out['decode_ms'] / out['windowed_ms'], 2)
    out['causal_over_windowed'] = round(out['causal_ms'] / out['windowed_ms'], 3)
    out['windowed_tokens_per_s'] = round(out['scored_tokens'] / (out['windowed_ms'] * 1e-3), 1)
    for k in ('windowed_ms', 'decode_ms', 'causal_ms'):
        out[k] = round(out[k], 3)
    for k in ('windowed_ms_runs', 'causal_ms_runs'):
        out[k] = [round(v, 3) for v in out[k]]
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
