"""Stage-2 generation PAST the 2048-token window, re-anchored (window='rebase') against windowed (window='device'), at the benchmark shape of
bench_stage2_window.py (d 512, 12 layers, 8 heads, d_ff 2048, V = 327, bf16, seeded random weights, its synthetic vocabulary, model and lead
sheets), Performer (128 features) and GPT-2, 32 streams of 120-bar lead sheets.  After the in-window device loop has handed the streams off,
on the SAME handed-off streams in ONE process:
  rebase   RebaseLoop: emo_acc_rebase + one variable-length prefill per phase, then the cached one-token step (grammar launch + engine step,
           replayed graphs) until the window is full again; --phases phases.  accepted draws / s, ms per token step, and the share of the
           time spent in the rebase launches, in the prefills, in graph captures (with the eager steps around them) and in the replays
  device   WindowedLoop: one batched [m, 2048] forward per draw; --steps steps.  accepted draws / s
`rebase_over_device` is the ratio of the two rates.  `state_error`: the error of emo_favor_state_at against float64 next to the forward's own
(the pair tests/test_gpu_favor_state_at.py asserts on, at its shape).  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from bench_stage2_gen import D, DFF, H, L, NF, TEMP, TOP_P, V, batch, model, vocab  # noqa: E402
from bench_stage2_window import device_phase  # noqa: E402


def rebase_phase(inf, loop, seed, keep, phases):
    rl = inf.RebaseLoop(loop, seed, keep)
    torch.cuda.synchronize()
    rl.run(max_phases=phases)
    acc, sec = rl.accepted_draws(), sum(rl.seconds.values())
    return dict(streams=rl.m0, phases=rl.phases, steps=rl.steps, accepted_draws=acc, seconds=round(sec, 4), draws_per_s=round(acc / sec, 1),
                ms_per_step=round(1e3 * sec / max(rl.steps, 1), 4), prefill_tokens=rl.prefill_tokens, persistent=rl.eng.persist is not None,
                share={k: round(v / sec, 4) for k, v in rl.seconds.items()})


def state_error():
    """The figures of tests/test_gpu_favor_state_at.py (its shape, seed and lengths): the largest |error| of emo_favor_state_at's S and z against
    float64, next to that of the forward's own state (favor_attn_fwd(want_state=True) on each row cut to its length) against the same float64."""
    import math
    from emo_disentanger_amd import ops
    B, H, DH, NF, T = 3, 2, 64, 128, 96
    gen = torch.Generator().manual_seed(11)
    k = torch.randn(B, T, H, DH, generator=gen) * 0.7
    v = torch.randn(B, T, H, DH, generator=gen)
    om = torch.randn(DH, NF // 2, generator=gen)
    out = {}
    for name, dt in (('bf16', torch.bfloat16), ('fp32', torch.float32)):
        kd, vd = k.to(dt), v.to(dt)
        kg, vg, og = kd.reshape(B * T, H * DH).cuda().contiguous(), vd.reshape(B * T, H * DH).cuda().contiguous(), om.cuda().contiguous()
        x = kd.double().permute(0, 2, 1, 3) * DH ** -0.25                                       # [B, H, T, dh]
        u, off = x @ om.double(), 0.5 * (x ** 2).sum(-1, keepdim=True) + 0.5 * math.log(NF)
        phi = torch.cat([torch.exp(u - off), torch.exp(-u - off)], -1)                         # [B, H, T, F]
        worst = {'state_at_S': 0.0, 'state_at_z': 0.0, 'forward_S': 0.0, 'forward_z': 0.0}
        for lens in ([1, 33, 96], [31, 32, 64]):
            S, z = ops.favor_state_at(kg, vg, og, torch.tensor(lens, dtype=torch.int32, device='cuda'), B, T, H)
            for b, n in enumerate(lens):
                Sr = phi[b, :, :n].transpose(-1, -2) @ vd.double().permute(0, 2, 1, 3)[b, :, :n]
                zr = phi[b, :, :n].sum(1)
                kb, vb = kg.view(B, T, H * DH)[b, :n], vg.view(B, T, H * DH)[b, :n]
                _, _, Sp, zp = ops.favor_attn_fwd(kb, kb, vb, og, 1, n, H, want_state=True)
                for key, got, ref in (('state_at_S', S[b], Sr), ('state_at_z', z[b], zr), ('forward_S', Sp[0], Sr), ('forward_z', zp[0], zr)):
                    worst[key] = max(worst[key], (got.cpu().double() - ref).abs().max().item())
        out[name] = {key: float('%.4g' % x) for key, x in worst.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=32)
    ap.add_argument('--bars', type=int, default=120)
    ap.add_argument('--phases', type=int, default=2)
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--rebase-keep', dest='rebase_keep', type=int, default=None)
    ap.add_argument('--kinds', default='performer,gpt2')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from emo_disentanger_amd import inference as inf
    torch.cuda.set_device(0)
    e2i, i2e = vocab()
    leads, primers = batch(e2i, args.streams, args.bars)
    W = inf.max_dec_inp_len
    keep = inf.check_rebase_keep(args.rebase_keep, W, max(len(p) for p in primers), max(len(b) for lead in leads for b in lead))
    out = {'tool': 'bench_stage2_rebase', 'shape': dict(d_model=D, n_layer=L, n_head=H, d_ff=DFF, V=V, performer_features=NF, dtype='bf16'),
           'streams': args.streams, 'bars': args.bars, 'window': W, 'rebase_keep': keep, 'temp': TEMP, 'top_p': TOP_P}
    for kind in args.kinds.split(','):
        m = model(kind, e2i)
        loop = inf.AccompanimentLoop(m, e2i, i2e, leads, primers, temp=TEMP, top_p=TOP_P, seed=1)
        loop.run(use_graph=True)
        r = {'in_window': dict(steps=loop.steps(), persistent=loop.eng.persist is not None, **loop.counts())}
        if r['in_window']['window'] == 0:
            raise SystemExit('no stream reached the window: raise --bars')
        rebase_phase(inf, loop, 1, keep, 1)                                 # warm-up (the prefill's shapes, the kernels' first launches)
        r['rebase'] = rebase_phase(inf, loop, 1, keep, args.phases)
        device_phase(inf, loop, 1, 16)                                      # warm-up of the [m, W] shapes
        r['device'] = device_phase(inf, loop, 1, args.steps)
        r['rebase_over_device'] = round(r['rebase']['draws_per_s'] / r['device']['draws_per_s'], 2)
        out[kind] = r
        del loop, m
        torch.cuda.empty_cache()
    out['state_error'] = state_error()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, 'w').write(line + '\n')
    print(line, flush=True)


if __name__ == '__main__':
    main()
