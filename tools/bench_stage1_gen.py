"""Stage-1 lead-sheet generation at the emopia_finetune.yaml shape (d 512, 12 layers, 8 heads, d_ff 2048, V = 200, bf16, mem_len = tgt_len
= 512, seeded random weights, a 200-event vocabulary of the stage-1 kinds): the reference-shaped single-stream loop generate_plain_xl
against the device loop generate_lead_sheets at 1 and 32 streams (grammar launch + decode_step per token step, hipGraph replays).
Prints one JSON line.  Roofline figure: the weight bytes one token step streams (from the shapes) over the step time.
Arguments: --events N (max_events per piece, default 512), --single-events N (default 256), --loop-only (the 32-stream device loop alone:
the run a kernel-trace profile is taken of), --step chain | one-launch | both (the model step of the device loop: decode_step's chain of
launches, the one persistent launch emo_decode_step (form 2), or both timed in this process on the same seeds: keys streams_N_one_launch and
one_launch_vs_chain_32_streams = chain ms per step / one-launch ms per step)."""
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
    ap.add_argument('--step', default='chain', choices=['chain', 'one-launch', 'both'])
    args = ap.parse_args()
    steps_timed = ['chain', 'one_launch'] if args.step == 'both' else [args.step.replace('-', '_')]
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
        res, sec = s1.generate_lead_sheets(m, e2i, i2e, primers, max_events=args.events, seed=1, step=steps_timed[-1], **kw)
        print(json.dumps({'tool': 'bench_stage1_gen', 'loop_only': True, 'step': steps_timed[-1], 'streams': 32, 'seconds': round(sec, 4),
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

    wb = weight_bytes_per_step()
    keys = []
    for n in (1, 32):
        primers = [['Emotion_%s' % emos[i % 6]] for i in range(n)]
        for step in steps_timed:
            s1.generate_lead_sheets(m, e2i, i2e, primers, max_events=32, seed=99, step=step, **kw)        # warm-up (kernels, workspaces)
            loop = s1.LeadSheetLoop(m, e2i, i2e, primers, max_events=args.events, seed=1, step=step, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.run(use_graph=True)
            sec = time.perf_counter() - t0
            steps = loop.pos - loop.L0
            acc = loop.accepted_tokens()
            res = loop.results()
            key = 'streams_%d' % n + ('' if step == 'chain' else '_one_launch')
            keys.append(key)
            out[key] = dict(steps=steps, accepted_tokens=acc, seconds=round(sec, 4), ms_per_step=round(1e3 * sec / steps, 4),
                            tokens_per_s=round(acc / sec, 1), finished=sum(isinstance(r, list) for r in res), stuck=sum(r is None for r in res))
            del loop
    out['weight_bytes_per_step'] = wb
    for key in keys:
        r = out[key]
        r['weight_tbps'] = round(wb / (r['ms_per_step'] * 1e-3) / 1e12, 3)
        r['roofline_fraction'] = round(r['weight_tbps'] / HBM_TBPS, 4)
    out['roofline_ms_per_step'] = round(wb / (HBM_TBPS * 1e12) * 1e3, 4)
    if 'streams_32' in out:
        out['speedup_32_streams_vs_single'] = round(out['streams_32']['tokens_per_s'] / out['single']['tokens_per_s'], 2)
    if args.step == 'both':
        out['one_launch_vs_chain_32_streams'] = round(out['streams_32']['ms_per_step'] / out['streams_32_one_launch']['ms_per_step'], 3)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
