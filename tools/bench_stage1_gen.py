"""Stage-1 lead-sheet generation at the emopia_finetune.yaml shape (d 512, 12 layers, 8 heads, d_ff 2048, V = 200, bf16, mem_len = tgt_len
= 512, seeded random weights, a 200-event vocabulary of the stage-1 kinds): the reference-shaped single-stream loop generate_plain_xl
against the device loop generate_lead_sheets at 1 and 32 streams (grammar launch + decode_step per token step, hipGraph replays).
Prints one JSON line.  Roofline figure: the weight bytes one token step streams (from the shapes) over the step time.
Arguments: --events N (max_events per piece, default 512), --single-events N (default 256), --loop-only (the 32-stream device loop alone:
the run a kernel-trace profile is taken of)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

D, L, H, DFF, V, TGT = 512, 12, 8, 2048, 200, 512
HBM_TBPS = 8.0                      # MI355X peak HBM bandwidth


def vocab():
    names = (['Emotion_%s' % e for e in ('Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative')]
             + ['Key_%s' % k for k in ('C', 'C#', 'D', 'D#', 'E', 'F', 'F#', 'G', 'G#', 'A', 'A#', 'B')]
             + ['Key_%s' % k for k in ('c', 'c#', 'd', 'd#', 'e', 'f', 'f#', 'g', 'g#', 'a', 'a#', 'b')]
             + ['Bar_None'] + ['Beat_%d' % i for i in range(16)] + ['Tempo_%d' % t for t in range(60, 180, 10)])
    names += ['Chord_%d_%d' % (i // 8, i % 8) for i in range(88)]
    names += ['Note_Degree_%d' % i for i in range(V - 2 - len(names))] + ['EOS_None', 'PAD_None']
    return {e: i for i, e in enumerate(names)}, dict(enumerate(names))


def weight_bytes_per_step(elem=2):
    per_layer = 3 * D * D + D * D + 2 * D * DFF                 # qkv_net, o_net, CoreNet.0 / .3 (the cached R rows are not weights)
    return elem * (L * per_layer + D * V)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--events', type=int, default=512)
    ap.add_argument('--single-events', type=int, default=256)
    ap.add_argument('--loop-only', action='store_true')
    args = ap.parse_args()
    from emo_disentanger_amd import stage1_inference as s1
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    m = PlainTransformer(D, V, L, H, D, DFF, TGT, TGT, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16').cuda().eval()
    e2i, i2e = vocab()
    emos = ['Q1', 'Q2', 'Q3', 'Q4', 'Positive', 'Negative']
    kw = dict(max_bars=128, temp=1.2, top_p=0.97, representation='functional', key_determine=None)
    out = {'tool': 'bench_stage1_gen', 'shape': dict(d_model=D, n_layer=L, n_head=H, d_ff=DFF, V=V, mem_len=TGT, dtype='bf16'), 'max_events': args.events}

    if args.loop_only:
        primers = [['Emotion_%s' % emos[i % 6]] for i in range(32)]
        res, sec = s1.generate_lead_sheets(m, e2i, i2e, primers, max_events=args.events, seed=1, **kw)
        print(json.dumps({'tool': 'bench_stage1_gen', 'loop_only': True, 'streams': 32, 'seconds': round(sec, 4),
                          'finished': sum(isinstance(r, list) for r in res)}), flush=True)
        return
    # single stream, the reference's loop: one model.generate per token, logits to the host, NumPy nucleus
    s1.generate_plain_xl(m, e2i, i2e, primer=['Emotion_Q1'], max_events=16, **kw)          # warm-up
    np.random.seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ids, _ = s1.generate_plain_xl(m, e2i, i2e, primer=['Emotion_Q1'], max_events=args.single_events, **kw)
    sec = time.perf_counter() - t0
    acc = len(ids) if ids is not None else 0                     # accepted words = tokens minus the 1-token primer = len(tokens[:-1])
    out['single'] = dict(accepted_tokens=acc, seconds=round(sec, 4), tokens_per_s=round(acc / sec, 1), ms_per_token=round(1e3 * sec / max(acc, 1), 4))

    for n in (1, 32):
        primers = [['Emotion_%s' % emos[i % 6]] for i in range(n)]
        s1.generate_lead_sheets(m, e2i, i2e, primers, max_events=32, seed=99, **kw)        # warm-up (kernels, workspaces)
        loop = s1.LeadSheetLoop(m, e2i, i2e, primers, max_events=args.events, seed=1, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run(use_graph=True)
        sec = time.perf_counter() - t0
        steps = loop.pos - loop.L0
        acc = loop.accepted_tokens()
        res = loop.results()
        out['streams_%d' % n] = dict(steps=steps, accepted_tokens=acc, seconds=round(sec, 4), ms_per_step=round(1e3 * sec / steps, 4),
                                     tokens_per_s=round(acc / sec, 1), finished=sum(isinstance(r, list) for r in res),
                                     stuck=sum(r is None for r in res))
        del loop
    wb = weight_bytes_per_step()
    out['weight_bytes_per_step'] = wb
    for n in (1, 32):
        r = out['streams_%d' % n]
        r['weight_tbps'] = round(wb / (r['ms_per_step'] * 1e-3) / 1e12, 3)
        r['roofline_fraction'] = round(r['weight_tbps'] / HBM_TBPS, 4)
    out['roofline_ms_per_step'] = round(wb / (HBM_TBPS * 1e12) * 1e3, 4)
    out['speedup_32_streams_vs_single'] = round(out['streams_32']['tokens_per_s'] / out['single']['tokens_per_s'], 2)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
