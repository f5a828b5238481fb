#!/usr/bin/env python3
"""bench.py — training tokens/s of the stage-2 Performer (d512, L12, H8, F128, seq 2048, bf16) on
synthetic EMOPIA-shaped batches: BASELINE.json configs[1] at N=1, configs[2] (DP over RCCL) at N>1.

One "step" = zero_grad + forward + CE loss + backward + grad all-reduce (N>1) + clip(0.5) + Adam +
LR schedule + device-side accuracy counts, with dropout 0.1 active and omega redrawn every forward
(reference-faithful).  Prints ONE JSON line on rank 0.

A plain run sets up, warms up, times `--steps` steps and prints the line; `--dump-outputs DIR` also writes
what the last timed step handed its caller (see dump_outputs).  `--full` adds everything else the line
can carry, each leg switched off again by its `--no-*` option: `roofline` (dominant kernel, HIP-event
timed on the launch stream), package power over the timed steps, `step0_check` against the CPU oracle
(before the timed steps), the generation, batch-4, fp32-parity, stage-1 and GPT-2 legs, and
`cpu_baseline` (the oracle's CPU training step timed on the host's cores; N=1 only).
"""
import argparse
import json
import math
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')

import torch  # noqa: E402

CFG = dict(n_token=327, n_layer=12, n_head=8, d_model=512, d_ff=2048, n_feat=128, seq=2048)
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


def gemm_flops_per_token():
    d, f, L, V = CFG['d_model'], CFG['d_ff'], CFG['n_layer'], CFG['n_token']
    return 3 * (L * 2 * (4 * d * d + 2 * d * f) + 2 * d * V)      # fwd + dgrad + wgrad = 227.5 MFLOP


def time_kernel(fn, iters=10, warm=3):
    """Average duration (ms) of `fn` (launches on torch's current stream) measured with HIP events on that stream."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


GEMM_KERNELS = {   # class of ops.gemm (one per kernel INSTANCE of the rocprofv3 summary) -> (kernel name, what it computes)
    'TN/rs': ('gemm_w128_tn_kernel<1> (256x256 tile, one wave per SIMD, bias gradient by ones-MFMAs) + splitk_reduce_kernel',
              'wgrad dW = dY^T X with the bias gradient, reduction over the B*T tokens: FFN1 and the fused QKV projection'),
    'TN/plain': ('gemm_w128_tn_kernel<0> (256x256 tile, one wave per SIMD) + splitk_reduce_kernel',
                 'wgrad dW = dY^T X (bias gradient taken by the LayerNorm backward): FFN2 and the 512x512 out-projection'),
    'TN/128': ('gemm_bf16_kernel<false,false,false,float,64,RS> + splitk_reduce_kernel', 'wgrad of outputs that are not multiples of 256 (the logits layer)'),
    'NN': ('gemm_bf16_glds_kernel<true,false,bf16,32,2>', 'dgrad dX = dY W (shapes outside the NT classes)'),
    'NT': ('gemm_bf16_glds_kernel<true,true,bf16,32,3>', 'forward Y = X W^T + fused epilogue, K = 512 (shapes outside the A-stationary class)'),
    'NT/K=512/plain': ('gemm_astat_kernel<bf16,0> (A stationary in registers, weights through the LDS ring)', 'K = 512, bias-only epilogue: QKV forward, out-projection dgrad'),
    'NT/K=512/relu+drop+mask': ('gemm_astat_kernel<bf16,19>', 'K = 512: FFN1 forward with ReLU + dropout + 1-bit mask output'),
    'NT/K=512/hdiv': ('gemm_astat_kernel<bf16,256>', 'K = 512, N = 512: out-projection dgrad leaving dN = dout / den (per-row, per-head divisor in the epilogue)'),
    'NT/K=512/bits': ('gemm_astat_kernel<bf16,8>', 'K = 512: FFN2 dgrad through the 1-bit relu.dropout mask'),
    'NT/K=512/drop+res': ('gemm_astat_kernel<bf16,6>', 'K = 512, N = 512: out-projection forward with dropout + residual (HBM-bound)'),
    'NT/K=512': ('gemm_astat_kernel<bf16,FL> (other epilogue instances)', 'K = 512 products'),
    'NT/K>1024': ('gemm_w128_kernel<bf16> (256x256 tile, one wave per SIMD, 128x128 quadrant per wave)',
                  'long reductions: FFN2 forward (K = 2048, bias + dropout + residual) and the FFN1 / QKV dgrads (K = 2048 / 1536) as NT products against transposed weight mirrors'),
}


def gemm_kernel_label(kind):
    k = kind
    while k and k not in GEMM_KERNELS:
        k = k.rsplit('/', 1)[0] if '/' in k else ''
    return GEMM_KERNELS.get(k, (kind, 'other GEMM'))


class PowerSampler(threading.Thread):
    """Package power (W) and shader clock (MHz) of the busiest amdgpu card the process can see, from the hwmon files, ~50 Hz: the GEMM phases of
    the step run at the package power limit with the clock pulled down, so the datasheet MFMA peak is not what a kernel can hold."""

    def __init__(self):
        super().__init__(daemon=True)
        import glob
        self.hw = []
        for h in glob.glob('/sys/class/drm/card*/device/hwmon/hwmon*'):
            pw = next((q for q in (h + '/power1_average', h + '/power1_input') if os.path.exists(q)), None)
            if pw and os.path.exists(h + '/freq1_input'):
                self.hw.append((pw, h + '/freq1_input', h + '/power1_cap'))
        self.rows, self.alive = [], True

    def run(self):
        while self.alive:
            best = None
            for pw, ck, cap in self.hw:
                try:
                    v = (int(open(pw).read()) / 1e6, int(open(ck).read()) / 1e6, int(open(cap).read()) / 1e6 if os.path.exists(cap) else None)
                except Exception:
                    continue
                if best is None or v[0] > best[0]:
                    best = v
            if best:
                self.rows.append(best)
            time.sleep(0.02)

    def result(self):
        self.alive = False
        r = self.rows[len(self.rows) // 4:]                      # (the first quarter of the window: clocks still settling)
        if not r:
            return None
        return {'package_w_avg': round(sum(x[0] for x in r) / len(r), 1), 'package_w_max': round(max(x[0] for x in r), 1), 'cap_w': r[0][2],
                'sclk_mhz_avg': round(sum(x[1] for x in r) / len(r)), 'samples': len(r),
                'note': 'hwmon power1_average / freq1_input sampled over the timed steps; sustained single-GEMM runs sit at the cap with sclk 1.65-2.0 GHz (tools/sustained_gemm.py)'}


def dominant_kernel_roofline(step_fn, B, T, n_steps=2):
    """Every GEMM launch inside `n_steps` real training steps is bracketed by HIP events on its launch stream (in situ: same data,
    same cache state as the timed region).  The GEMM kernel classes (wgrad TN, A-stationary NT at K=512, long-reduction NT: FFN2 forward + dgrads) take ~65 % of the
    step; `roofline` is the kernel INSTANCE with the largest total time (= the first line of the rocprofv3 summary under profiles/),
    the others are listed in `roofline_others`.  achieved = sum(algorithmic FLOPs = 2*M*N*K) / sum(durations).

    Kernel durations only mean something when kernels do not share the CUs: the optional second HIP stream for wgrad
    (EMO_WGRAD_STREAM=1, off by default) is forced off for the instrumented steps; when it is enabled for the timed region the
    stretched in-step average is reported next to the serialized one."""
    from emo_disentanger_amd import engine, ops

    extra = {}

    def instrumented(side_on):
        was, was_auto = engine._SIDE['on'], engine._SIDE['auto']
        engine._SIDE['on'] = side_on and was
        engine._SIDE['auto'] = side_on and was_auto            # (kernel durations only mean something when kernels do not share the CUs)
        ops.GEMM_TIMING, ops.KERNEL_TIMING = [], {}
        try:
            for _ in range(n_steps):
                step_fn()
            torch.cuda.synchronize()
        finally:
            rec, ops.GEMM_TIMING = ops.GEMM_TIMING, None
            other, ops.KERNEL_TIMING = ops.KERNEL_TIMING, None
            engine._SIDE['on'], engine._SIDE['auto'] = was, was_auto
        extra.clear()
        extra.update(other)
        by = {}
        for kind, e0, e1, fl, by_ in (r[:5] for r in rec):
            d = by.setdefault(kind, {'ms': 0.0, 'flops': 0.0, 'bytes': 0.0, 'n': 0})
            d['ms'] += e0.elapsed_time(e1); d['flops'] += fl; d['bytes'] += by_; d['n'] += 1
        return by

    serial = instrumented(False)
    overlapped = instrumented(True) if engine._SIDE['on'] else {}
    # PMC counters of THIS round's kernels inside the training step (tools/pmc_step.py under rocprofv3 --pmc, one counter group per pass,
    # summarised by tools/pmc_classes.py): HBM bytes per launch and the MFMA pipe's busy fraction per kernel class
    # — printed ONLY while the file's stamp (hash of the kernel sources it was collected with) matches the sources of this run: stale counters
    # are dropped, not shown (r02 printed counters of kernels that no longer existed)
    pmc_all, pmc_note = load_pmc()

    def entry(kind):
        d = serial[kind]
        achieved = d['flops'] / d['ms'] / 1e9
        pmc = (pmc_all.get(kind) or pmc_all.get(kind.rsplit('/', 1)[0], {})) if B * T == 131072 else {}     # (collected at the bench shape only)
        traffic = pmc.get('traffic_bytes_per_launch')
        if kind.startswith('TN') and traffic is not None and 'TN-reduce' in pmc_all:     # split-K partial sums + their reduce launch belong to the wgrad class
            traffic += pmc_all['TN-reduce'].get('traffic_bytes_per_launch', 0)
        return {'bound': 'mfma', 'achieved': round(achieved, 1), 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s',
                'frac': round(achieved / PEAK_BF16_TFLOPS, 4), 'traffic': traffic, 'mfma_busy': pmc.get('mfma_busy'),
                'waves_parked': pmc.get('waves_parked'), 'waves_issue_stalled': pmc.get('waves_issue_stalled'), 'effective_clock_ghz': pmc.get('effective_clock_ghz'),
                'kernel': '%s (%s)' % gemm_kernel_label(kind), 'launches_timed': d['n'], 'avg_launch_ms': round(d['ms'] / d['n'], 4),
                'total_ms_per_step': round(d['ms'] / n_steps, 2),
                'avg_launch_ms_overlapped_in_step': round(overlapped[kind]['ms'] / overlapped[kind]['n'], 4) if kind in overlapped else None,
                'algorithmic_flops_per_launch': round(d['flops'] / d['n']), 'algorithmic_bytes_per_launch': round(d['bytes'] / d['n'])}

    order = sorted(serial, key=lambda k: -serial[k]['ms'])
    roof = entry(order[0])
    fam = {}
    for k_, d_ in serial.items():                       # the instances of one kernel family taken together (A-stationary: 4 epilogue instances; wgrad: 3 kernels)
        f_ = fam.setdefault('/'.join(k_.split('/')[:2]) if k_.startswith('NT') else k_.split('/')[0], {'ms': 0.0, 'flops': 0.0})
        f_['ms'] += d_['ms']; f_['flops'] += d_['flops']
    roof['gemm_families'] = {k_: {'achieved_tflops': round(f_['flops'] / f_['ms'] / 1e9, 1), 'frac': round(f_['flops'] / f_['ms'] / 1e9 / PEAK_BF16_TFLOPS, 4),
                                  'total_ms_per_step': round(f_['ms'] / n_steps, 2)} for k_, f_ in sorted(fam.items(), key=lambda kv: -kv[1]['ms'])}
    roof['timing'] = 'HIP events on the launch stream around every GEMM launch in %d real training steps (kernels serialized on one stream)' % n_steps
    import glob
    summaries = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', 'r*_bench_train_rocprof_stats.txt')))
    roof['rocprof_summary'] = ('profiles/%s = rocprofv3 --kernel-trace --stats of `bench.py --full --steps 10 --warmup 3 --no-cpu-baseline '
                               % (os.path.basename(summaries[-1]) if summaries else '(none committed)') +
                               '--no-gen --no-stage1 --no-gpt2 --no-step0-check --no-b4 --no-fp32` (training kernels only); PMC (traffic, mfma_busy, effective clock): ' + pmc_note)
    roof['roofline_others'] = [entry(k) for k in order[1:]] + [attn_entry(k, v, n_steps, pmc_all if B * T == 131072 else {}) for k, v in sorted(extra.items())]
    return roof


ATTN_KERNELS = {'ffn_fused_fwd': ('ffn_fused_fwd_kernel (LayerNorm1 -> FFN1 -> ReLU -> dropout -> FFN2 -> dropout -> + residual in one launch; one workgroup per CU, hidden chunk handed from the FFN1 accumulators into the FFN2 MFMAs)', 'mfma', 'the feed-forward block of a layer, forward: 2 x 2 M 512 2048 flop; bytes = x1 read + h1, f, mask, x2 written'),
                'favor_fwd': ('favor_fs_fwd_kernel (bf16 slice kernel; generic: favor_fwd_kernel)', 'hbm', 'FAVOR+ causal linear attention forward: features + chunked prefix-sum scan; bytes = q, k, v read + out written (4*512*e per token*layer)'),
                'favor_bwd': ('favor_fs_dq_kernel + favor_fs_dkv_kernel (bf16 slice kernels; generic: favor_bwd_dq_kernel / favor_bwd_dkv_kernel)', 'hbm', 'FAVOR+ backward (forward sweep dq, reverse sweep dk/dv); bytes = 7*512*e per token*layer'),
                'sattn_fwd': ('sattn32_fwd_kernel (32x32x16 tiles; generic: sattn_fwd_kernel)', 'mfma', 'GPT-2 causal softmax attention forward (flash tiles): 2 matmuls, causal half'),
                'sattn_bwd': ('sattn32_dq_kernel + sattn32_dkv_kernel (32x32x16 tiles, dropout keep bits from the forward; generic: sattn_bwd_dq_kernel + sattn_bwd_dkv_kernel)', 'mfma', 'GPT-2 attention backward: 7 matmuls, causal half')}


def load_pmc():
    """(classes, note): the newest profiles/r*_pmc_step.json whose csrc_hash equals the hash of the kernel sources in this tree."""
    import glob
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        from pmc_classes import csrc_hash
        now = csrc_hash()
    except Exception as e:   # noqa: BLE001
        return {}, 'no PMC file used (%s)' % e
    for path in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_step.json')), reverse=True):
        j = json.load(open(path))
        if j.get('csrc_hash') == now:
            return j['classes'], '%s (stamp %s = the kernel sources of this run)' % (os.path.relpath(path, ROOT), now)
    return {}, 'no PMC file matches the kernel sources of this run (hash %s): traffic / mfma_busy / clock omitted — re-run tools/collect_profiles.sh' % now


def attn_entry(kind, rec, n_steps, pmc_all=None):
    """roofline entry of an attention kernel class from in-situ HIP-event brackets (ops._timed)."""
    pmc_all = pmc_all or {}
    parts = [pmc_all[k] for k in ((kind,) if kind != 'favor_bwd' else ('favor_bwd_dq', 'favor_bwd_dkv')) if k in pmc_all]
    traffic = sum(p.get('traffic_bytes_per_launch', 0) for p in parts) if parts and all('traffic_bytes_per_launch' in p for p in parts) else None
    ms = sum(e0.elapsed_time(e1) for e0, e1, _, _ in rec)
    fl, by = sum(r[2] for r in rec), sum(r[3] for r in rec)
    name, bound, what = ATTN_KERNELS[kind]
    if bound == 'hbm':
        ach, peak, unit = by / ms / 1e6, PEAK_HBM_GBS, 'GB/s'
    else:
        ach, peak, unit = fl / ms / 1e9, PEAK_BF16_TFLOPS, 'TFLOP/s'
    return {'bound': bound, 'achieved': round(ach, 1), 'peak': peak, 'unit': unit, 'frac': round(ach / peak, 4), 'traffic': traffic,
            'mfma_busy': [p.get('mfma_busy') for p in parts] if parts else None, 'effective_clock_ghz': [p.get('effective_clock_ghz') for p in parts] if parts else None, 'lds_conflict_share': [p.get('lds_conflict_share') for p in parts] if parts else None,
            'kernel': '%s (%s)' % (name, what),
            'launches_timed': len(rec), 'avg_launch_ms': round(ms / len(rec), 4), 'total_ms_per_step': round(ms / n_steps, 2),
            'algorithmic_flops_per_launch': round(fl / len(rec)), 'algorithmic_bytes_per_launch': round(by / len(rec))}


def gpt2_bench(n_steps=6, B=16, T=2048):
    """Secondary line: the GPT-2 backbone of the same hot path (north_star: masked-softmax attention) at the pop1k7_pretrain_gpt2 shape
    (d512 / L12 / H8), B=16 x T=2048, bf16, dropout 0.1, fwd + bwd + clip + fused Adam on synthetic tokens; the flash-attention kernels are
    timed in situ with HIP events."""
    import contextlib
    from emo_disentanger_amd import ops
    from emo_disentanger_amd.data import synthetic_batch
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    from emo_disentanger_amd.optim import FusedAdam
    with contextlib.redirect_stdout(sys.stderr):
        m = MusicGPT2(CFG['n_token'], 12, 8, 512, 2048, 512, use_segment_emb=True, n_segment_types=2, dropout=0.1, compute_dtype='bf16').cuda().train()
    opt = FusedAdam(m, lr=1e-5, max_grad_norm=0.5)
    b = synthetic_batch(CFG['n_token'], B, T, device='cuda')

    def step():
        opt.zero_grad()
        loss = m.compute_loss(m(b['dec_input'], seg_inp=b['track_mask']), b['dec_target'])['total_loss']
        loss.backward()
        opt.step()
        return loss
    for _ in range(5):                       # (7-ms steps: 5 untimed + 30 timed ones, so that clocks / allocator / launch queue are in steady state)
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n_steps
    ops.KERNEL_TIMING = {}
    try:
        step()
        step()
        torch.cuda.synchronize()
    finally:
        rec, ops.KERNEL_TIMING = ops.KERNEL_TIMING, None
    return {'metric': 'GPT-2 backbone train tokens/sec', 'value': round(B * T / dt, 1), 'unit': 'tokens/s', 'ms_per_step': round(dt * 1e3, 3),
            'config': {'workload': 'stage2 GPT-2 d512 L12 H8 d_ff2048, B=%d x T=%d, bf16, dropout 0.1 (attention-probability dropout in-kernel), fused Adam' % (B, T)},
            'loss': round(float(loss.detach()), 4), 'roofline': [attn_entry(k, v, 2) for k, v in sorted(rec.items())]}


def generation_bench(model, n_streams=32, prompt=64, n_new=2048 - 64, top_p=0.9, temp=1.1):
    """BASELINE configs[3]: 32 parallel streams, 64-token prompt, generate to 2048 tokens, nucleus p=0.9, recurrent FAVOR+ state in HBM,
    hipGraph-replayed decode step; tokens/s = streams * new tokens / wall time (engine set-up, prefill of the prompt and graph capture included)."""
    from emo_disentanger_amd import inference as inf
    dev = next(model.parameters()).device
    g = torch.Generator().manual_seed(7)
    ptok = torch.randint(0, CFG['n_token'] - 1, (n_streams, prompt), generator=g).to(dev)
    pseg = torch.ones(n_streams, prompt, dtype=torch.long, device=dev)
    model.eval()
    inf.generate_streams(model, ptok, pseg, 8, temp=temp, top_p=top_p, seed=1)          # warm-up (kernels, graph machinery)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = inf.generate_streams(model, ptok, pseg, n_new, temp=temp, top_p=top_p, seed=2)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert out.shape == (n_streams, prompt + n_new) and int(out.max()) < CFG['n_token']
    # the reference's own use: ONE piece at a time (inference.py:231-327) — a single stream on the same engine (idle padding streams)
    inf.generate_streams(model, ptok[:1], pseg[:1], 8, temp=temp, top_p=top_p, seed=1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    inf.generate_streams(model, ptok[:1], pseg[:1], 512, temp=temp, top_p=top_p, seed=3)
    torch.cuda.synchronize()
    single_ms = 1000 * (time.perf_counter() - t1) / 512
    model.train()
    # roofline: a token step streams the bf16 matrices once for all streams and reads + writes every stream's FAVOR+ state
    # (12 layers x 8 heads x (128 x 64 + 128) fp32, read and written)
    wbytes = 2 * sum(p.numel() for n_, p in model.named_parameters() if p.dim() == 2 and 'emb' not in n_)
    sbytes = n_streams * CFG['n_layer'] * CFG['n_head'] * (CFG['n_feat'] * (CFG['d_model'] // CFG['n_head']) + CFG['n_feat']) * 4 * 2
    step_s = dt / n_new
    ach = (wbytes + sbytes) / step_s / 1e9
    return {'metric': 'AR gen tokens/sec, stage2 Performer d512 L12, %d streams, nucleus p=%.2f' % (n_streams, top_p),
            'value': round(n_streams * n_new / dt, 1), 'unit': 'tokens/s', 'streams': n_streams, 'prompt': prompt, 'new_tokens': n_new,
            'ms_per_token_step': round(1000 * dt / n_new, 3), 'single_stream_ms_per_token': round(single_ms, 3),
            'roofline': {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': round(ach / PEAK_HBM_GBS, 4),
                         'algorithmic_bytes_per_step': int(wbytes + sbytes),
                         'note': 'weights %.1f MB + recurrent state read and written %.1f MB per token step; the step is 60 dependent all-gather edges (latency), not bytes' % (wbytes / 1e6, sbytes / 1e6)},
            'engine': 'FAVOR+ recurrent state in HBM; token step = ONE persistent launch (emo_performer_decode_step_sampled: nucleus draw + embedding + 12 layers + logits), hipGraph replay'}


def gpt2_generation_bench(n_streams=32, prompt=64, n_new=2048 - 64, top_p=0.9, temp=1.1):
    """BASELINE configs[3] names a KV cache: the same 32 x 2048 nucleus generation on the GPT-2 backbone (d512 / L12 / H8) — head-major KV cache
    [n, 8, 2048, 64] x 2 per layer in HBM (bf16), token step = ONE persistent launch (emo_gpt2_decode_step_sampled, r06: nucleus draw, embedding,
    12 blocks with the softmax attention over the cache, logits), hipGraph-replayed; r05 and EMO_GPT2_PERSISTENT=0: a chain of launches (skinny
    GEMMs with the LayerNorms folded in, sattn_decode, nucleus sampler).  Roofline: HBM bytes a token step must move = the bf16 weights once +
    every stream's keys and values of all layers at the step's context length (12 x 2 x ctx x 512 x 2 B), averaged over the generated positions."""
    import contextlib
    from emo_disentanger_amd import inference as inf
    from emo_disentanger_amd.model.music_gpt2 import MusicGPT2
    with contextlib.redirect_stdout(sys.stderr):
        m = MusicGPT2(CFG['n_token'], 12, 8, 512, 2048, 512, use_segment_emb=True, n_segment_types=2, dropout=0.1, compute_dtype='bf16').cuda().eval()
    g = torch.Generator().manual_seed(7)
    ptok = torch.randint(0, CFG['n_token'] - 1, (n_streams, prompt), generator=g).cuda()
    pseg = torch.ones(n_streams, prompt, dtype=torch.long, device='cuda')
    inf.generate_streams(m, ptok, pseg, 8, temp=temp, top_p=top_p, seed=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = inf.generate_streams(m, ptok, pseg, n_new, temp=temp, top_p=top_p, seed=2)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert out.shape == (n_streams, prompt + n_new) and int(out.max()) < CFG['n_token']
    wbytes = 2 * sum(p.numel() for n_, p in m.named_parameters() if p.dim() == 2 and 'emb' not in n_)      # bf16 matrices read by a step
    ctx = prompt + (n_new + 1) / 2.0                                                                       # mean context length of a generated token
    kv = n_streams * 12 * 2 * ctx * 512 * 2
    step_s = dt / n_new
    ach = (wbytes + kv) / step_s / 1e9
    return {'metric': 'AR gen tokens/sec, stage2 GPT-2 d512 L12, %d streams, nucleus p=%.2f, KV cache in HBM' % (n_streams, top_p),
            'value': round(n_streams * n_new / dt, 1), 'unit': 'tokens/s', 'streams': n_streams, 'prompt': prompt, 'new_tokens': n_new,
            'ms_per_token_step': round(1000 * step_s, 3),
            'roofline': {'bound': 'hbm', 'achieved': round(ach, 1), 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': round(ach / PEAK_HBM_GBS, 4),
                         'algorithmic_bytes_per_step': int(wbytes + kv), 'note': 'weights %.1f MB + KV cache %.1f MB at the mean context of %d tokens' % (wbytes / 1e6, kv / 1e6, ctx)},
            'engine': 'head-major KV cache [n, 8, 2048, 64] x 2 x 12 layers (bf16) in HBM; token step = ' +
                      ('one persistent launch (emo_gpt2_decode_step_sampled: draw + embedding + 12 blocks + logits), hipGraph-replayed'
                       if os.environ.get('EMO_GPT2_PERSISTENT', '1') != '0' and os.environ.get('EMO_DECODE_PERSISTENT', '1') != '0'
                       else 'hipGraph replay of the launch chain (skinny GEMMs with folded LayerNorms, sattn_decode, nucleus sampler)')}


def stage1_bench(n_steps=30, B=4, T=512, V=200):
    """Secondary line, BASELINE configs[4] (single GPU): the stage-1 lead-sheet LM (Transformer-XL decoder, emopia_finetune.yaml shape:
    d512 / L12 / H8 / d_ff 2048, tgt_len 512, batch 4), bf16, dropout 0.1, fwd + bwd + clip + fused Adam on synthetic tokens."""
    from emo_disentanger_amd.model.plain_transformer import PlainTransformer
    from emo_disentanger_amd.optim import FusedAdam
    m = PlainTransformer(512, V, 12, 8, 512, 2048, 0, T, dec_dropout=0.1, pre_lnorm=True, compute_dtype='bf16').cuda().train()
    opt = FusedAdam(m, lr=1e-5, max_grad_norm=0.5)
    g = torch.Generator().manual_seed(1)
    x, tgt = torch.randint(0, V - 1, (T, B), generator=g).cuda(), torch.randint(0, V - 1, (T, B), generator=g).cuda()

    def step():
        opt.zero_grad()
        loss = m.compute_loss(m(x, tuple())[0], tgt)['total_loss']
        loss.backward()
        opt.step()
        return loss
    for _ in range(5):                       # (7-ms steps: 5 untimed + 30 timed ones, so that clocks / allocator / launch queue are in steady state)
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n_steps
    return {'metric': 'stage1 (Transformer-XL lead-sheet LM) train tokens/sec', 'value': round(B * T / dt, 1), 'unit': 'tokens/s', 'ms_per_step': round(dt * 1e3, 3),
            'config': {'workload': 'BASELINE configs[4] shape, 1 GPU: d512 L12 H8 d_ff2048 tgt_len=%d batch=%d V=%d, bf16, dropout 0.1' % (T, B, V)},
            'loss': round(float(loss), 4)}


def step0_check(model, batch):
    """Loss of the bench's OWN weights on the first sequence of its own batch, HIP path vs the CPU oracle (omega fixed, dropout 0, outside the
    timed region; SURVEY §8(d) "Timing protocol").  bf16 = the timed compute mode, fp32 = parity mode (north_star: |dloss| <= 1e-4)."""
    from oracle import model_ref
    x, seg, tgt = batch['dec_input'][:1], batch['track_mask'][:1], batch['dec_target'][:1]
    redraw, training = model.redraw, model.training
    model.redraw = 'fixed'
    model.eval()
    out = {}
    try:
        with torch.no_grad():
            for dt in ('fp32', 'bf16'):                         # (ends on bf16: the store of the timed run is rebuilt once)
                model.set_compute_dtype(dt)
                out['loss_hip_' + dt] = float(model.compute_loss(model(x, seg_inp=seg), tgt)['total_loss'])
            sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
            t0 = time.time()
            ref = model_ref.compute_loss(model_ref.forward('performer', sd, x.cpu(), seg.cpu(), CFG['n_layer'], CFG['n_head'], CFG['d_model']),
                                         tgt.cpu(), CFG['n_token'])
            out['loss_oracle'] = float(ref)
            out['oracle_seconds'] = round(time.time() - t0, 2)
    finally:
        model.redraw = redraw
        model.train(training)
    out['abs_err_fp32'] = abs(out['loss_hip_fp32'] - out['loss_oracle'])
    out['abs_err_bf16'] = abs(out['loss_hip_bf16'] - out['loss_oracle'])
    out['abs_err'] = out['abs_err_bf16']
    # north_star's bound (1e-4) is asserted for the fp32 parity mode; the timed bf16 mode is held to 3e-4 (the mean of 2048 signed per-token
    # errors of ~1e-2: its size moves with the summation order) and the line says whether it ALSO met 1e-4 on this sample
    out['bf16_meets_1e-4'] = bool(out['abs_err_bf16'] <= 1e-4)
    out['ok'] = bool(out['abs_err_fp32'] <= 1e-4 and out['abs_err_bf16'] <= 3e-4)
    out['sample'] = 'first sequence (B=1 x T=%d) of the timed batch, the timed weights, omega fixed, dropout 0' % x.shape[1]
    return out


def cpu_generation_baseline(ctx=256, n_tok=4):
    """Reference-style AR step on the CPU oracle: full-prefix recompute per token (inference.py:252-272), 1 stream."""
    from oracle import model_ref
    from oracle.weights import make_state_dict
    sd = make_state_dict('performer', CFG['n_token'], CFG['n_layer'], CFG['n_head'], CFG['d_model'], CFG['d_ff'], favor_feature_dims=CFG['n_feat'], seed=0)
    x = torch.randint(0, CFG['n_token'] - 1, (1, ctx))
    seg = torch.ones(1, ctx, dtype=torch.long)
    with torch.no_grad():
        model_ref.forward('performer', sd, x, seg, CFG['n_layer'], CFG['n_head'], CFG['d_model'], keep_last_only=True)
        t0 = time.time()
        for _ in range(n_tok):
            model_ref.forward('performer', sd, x, seg, CFG['n_layer'], CFG['n_head'], CFG['d_model'], keep_last_only=True)
        dt = (time.time() - t0) / n_tok
    return {'value': round(1.0 / dt, 2), 'unit': 'tokens/s', 'cores': torch.get_num_threads(), 'kind': 'port',
            'sample': 'oracle full-prefix recompute at context %d, 1 stream, %d tokens' % (ctx, n_tok)}


def cpu_baseline(T, steps=2):
    """Oracle (CPU restatement of the reference path: torch fp32 eager + the C causal-product) timed on the host cores: forward + loss +
    backward + clip(0.5) + Adam on B=1 x T tokens, all cores (`value`) and 8 threads (`value_8_threads`, the survey container's core count)."""
    from oracle import model_ref
    from oracle.weights import make_state_dict, synthetic_batch
    sd = make_state_dict('performer', CFG['n_token'], CFG['n_layer'], CFG['n_head'], CFG['d_model'], CFG['d_ff'], favor_feature_dims=CFG['n_feat'], seed=0)
    b = synthetic_batch(CFG['n_token'], 1, T, seed=1234)
    cores = torch.get_num_threads()
    args = ('performer', sd, b, CFG['n_token'], CFG['n_layer'], CFG['n_head'], CFG['d_model'])
    params = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items() if v.is_floating_point() and not k.endswith('pe.pe') and 'omega' not in k}
    opt = torch.optim.Adam(params.values(), lr=1e-4)

    def one_step():
        _, _, grads = model_ref.loss_and_grads(*args, p_drop=0.1, training=True)
        for k, p in params.items():
            p.grad = grads[k]
        torch.nn.utils.clip_grad_norm_(params.values(), 0.5)
        opt.step()
    one_step()                                                        # warm-up (also builds the C kernel)
    t0 = time.time()
    for _ in range(steps):
        one_step()
    dt = (time.time() - t0) / steps
    tried = {cores: round(T / dt, 1)}
    for nt in (32, 16, 8):                                              # the box oversubscribes at all cores (r02: 369 tok/s at 128 threads, 1359 at 8)
        if nt < cores:
            torch.set_num_threads(nt)
            os.environ['OMP_NUM_THREADS'] = str(nt)
            try:
                t0 = time.time()
                one_step()
                tried[nt] = round(T / (time.time() - t0), 1)
            finally:
                torch.set_num_threads(cores)
    best = max(tried, key=tried.get)
    return {'value': tried[best], 'unit': 'tokens/s', 'cores': best, 'kind': 'port', 'tokens_per_s_by_threads': {str(k): v for k, v in sorted(tried.items())},
            'sample': 'oracle Performer L12 d512 fwd + bwd + clip + Adam, B=1 x T=%d, torch fp32 eager + C causal product; %d timed steps at all %d '
                      'threads, one step at each smaller count; value = the best thread count tried' % (T, steps, cores)}


def dp_selftest(model, rank, world):
    """The gradient exchange of one optimizer step on a rank-stamped buffer: the flat gradient (152.7 MB fp32 at the bench config) is
    filled with (rank + 1) * pattern(i), sent through dp.GradExchange exactly as a training step does (late-layer range on the
    communication stream while the compute stream is busy, the rest + the token-count tail afterwards) and EVERY element is compared
    with world (world + 1) / 2 * pattern(i).  A broken overlap (missing stream dependency, wrong range) shows up as a wrong element
    here, not as a slightly wrong loss later.  Also times the exchange with HIP events (comm stream)."""
    from emo_disentanger_amd import dp
    ps = model._ensure_store()
    n = ps.total
    idx = torch.arange(n, device=ps.device, dtype=torch.float32)
    pattern = (idx % 251.0) * 0.5 + 1.0                         # exact in fp32, sums of <= 8 multiples stay exact
    ps.ensure_grads()
    ex = dp.GradExchange(model, ps)
    out = {'elements': int(n), 'bytes': int(4 * n), 'split': bool(ex.range is not None), 'plane': dp.data_plane()}
    times = []
    for rep in range(3):
        ps.flat_grad.copy_(pattern * float(rank + 1))
        busy = torch.randn(4096, 4096, device=ps.device)        # keeps the compute stream busy while the first piece is in flight
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        dp.barrier()
        e0.record()
        ex.arm()
        if ex.range is not None and ex._enabled():
            ex._on_layer(ex.range[2])                           # what DecoderStackFn.backward calls half-way through the sweep
        busy = busy @ busy
        ex.finish(torch.tensor(float(100 + rank), device=ps.device))
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        want_sum = world * (world + 1) / 2.0
        bad = int((ps.flat_grad != pattern * want_sum).sum())
        tail = float(ps.flat_grad_ext[ps.total])
        tail_want = float(sum(100 + r for r in range(world)))
        out.update(bad_elements=bad, tail=tail, tail_expected=tail_want)
        if bad or tail != tail_want:
            break
    ps.flat_grad.zero_()
    out['ok'] = bool(out['bad_elements'] == 0 and out['tail'] == out['tail_expected'])
    out['exchange_ms'] = round(min(times), 3)
    out['allreduce_GBps_per_gpu'] = round(4 * n / (min(times) * 1e-3) / 1e9, 1)
    return out


def b4_bench(model, opt_cls, tr, steps=30, warm=5):
    """SURVEY 8(d) cfg2 second batch size: the reference YAML's batch_size 4 (pop1k7_pretrain.yaml) through the same product loop."""
    import tempfile
    from emo_disentanger_amd.data import synthetic_batch
    B, T = 4, CFG['seq']
    dev = next(model.parameters()).device
    bs = [synthetic_batch(CFG['n_token'], B, T, seed=4321 + i, device=dev) for i in range(2)]
    cfg = tr.TrainConfig(warmup_steps=200, max_lr=1e-4, min_lr=1e-5, lr_decay_steps=500000, redraw_prob=1.0, log_interval=10 ** 9,
                         ckpt_dir=tempfile.mkdtemp(prefix='emo_bench_b4_'), verbose=False)
    opt = opt_cls(model, lr=1e-4, max_grad_norm=0.5)
    tr.train_model(1, model, [bs[i % 2] for i in range(warm)], opt, None, CFG['n_token'] - 1, cfg=cfg)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = tr.train_model(1, model, [bs[i % 2] for i in range(steps)], opt, None, CFG['n_token'] - 1, cfg=cfg)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {'metric': 'train tokens/sec at the reference YAML batch size', 'value': round(B * T / dt, 1), 'unit': 'tokens/s', 'ms_per_step': round(dt * 1e3, 3),
            'config': {'workload': 'stage2 Performer d512 L12 H8 F128 seq=%d, B=%d (pop1k7_pretrain.yaml batch_size), bf16, dropout 0.1, omega redraw every forward' % (T, B)},
            'mean_loss': round(loss, 4)}


PEAK_F32_TFLOPS = 157.3        # exact-f32 MFMA peak (v_mfma_f32_*_f32), /opt/skills/guides/cdna_hip_programming.md


def fp32_parity_bench(tr, opt_cls, B, T, steps=5, warm=3):
    """The mode in which north_star's tolerances are asserted (loss within 1e-4 of the CPU oracle, exact greedy ids: tests/test_gpu_model.py, step0_check)
    on the clock (r05 verdict): the SAME product loop (train.train_model, dropout 0.1, omega redrawn every forward, fused clip + Adam) with
    compute_dtype='fp32' — fp32 storage, exact-f32 MFMA products (v_mfma_f32_16x16x4_f32 = an fp32 FMA chain), fp32 FAVOR+ / LayerNorm / loss.
    B = the benchmark's batch when it fits, halved on an out-of-memory error.  Roofline: the model's GEMM flops per step against the 157.3-TFLOP/s
    exact-f32 MFMA peak (the fp32 kernels are the parity yardstick, not tuned: 64 x 64 x 16 tiles, register-staged)."""
    import contextlib
    import tempfile
    from emo_disentanger_amd.data import synthetic_batch
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    while B >= 1:
        try:
            with contextlib.redirect_stdout(sys.stderr):
                m = MusicPerformer(CFG['n_token'], CFG['n_layer'], CFG['n_head'], CFG['d_model'], CFG['d_ff'], CFG['d_model'], favor_feature_dims=CFG['n_feat'],
                                   use_segment_emb=True, n_segment_types=2, dropout=0.1, compute_dtype='fp32', redraw='every_forward').cuda().train()
            bs = [synthetic_batch(CFG['n_token'], B, T, seed=777 + i, device='cuda') for i in range(2)]
            cfg = tr.TrainConfig(warmup_steps=200, max_lr=1e-4, min_lr=1e-5, lr_decay_steps=500000, redraw_prob=1.0, log_interval=10 ** 9,
                                 ckpt_dir=tempfile.mkdtemp(prefix='emo_bench_fp32_'), verbose=False)
            opt = opt_cls(m, lr=1e-4, max_grad_norm=0.5)
            tr.train_model(1, m, [bs[i % 2] for i in range(warm)], opt, None, CFG['n_token'] - 1, cfg=cfg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = tr.train_model(1, m, [bs[i % 2] for i in range(steps)], opt, None, CFG['n_token'] - 1, cfg=cfg)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / steps
            break
        except torch.OutOfMemoryError:
            m = opt = bs = None
            torch.cuda.empty_cache()
            B //= 2
    else:
        return {'error': 'out of memory at B = 1'}
    tf = B * T * gemm_flops_per_token() / dt / 1e12
    return {'metric': 'train tokens/sec in the fp32 parity mode', 'value': round(B * T / dt, 1), 'unit': 'tokens/s', 'ms_per_step': round(dt * 1e3, 3), 'steps': steps, 'warmup': warm,
            'dtype': 'f32', 'config': {'workload': 'stage2 Performer d512 L12 H8 F128 seq=%d, B=%d, compute_dtype=fp32 (exact-f32 MFMA), dropout 0.1, omega redraw every forward, '
                                                   'fwd+bwd+clip+Adam through train.train_model' % (T, B)},
            'mean_loss': round(loss, 4),
            'roofline': {'bound': 'mfma', 'achieved': round(tf, 1), 'peak': PEAK_F32_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(tf / PEAK_F32_TFLOPS, 4),
                         'note': 'GEMM flops of the model per step (227.5 MFLOP per token) / whole step time, against the exact-f32 MFMA peak'},
            'tolerances': 'this is the mode whose loss is within 1e-4 of the CPU oracle and whose greedy ids are exact (step0_check.abs_err_fp32, '
                          'tests/test_gpu_model.py::test_performer_at_benchmark_shape_matches_oracle[fp32-*])'}


DUMP_SAMPLE = 1 << 22          # elements per sampled array: 2 x 16 MB of fp32


def dump_outputs(model, mean_loss, out_dir, seed=0):
    """What the timed path (train.train_model) hands its caller after the last timed step, as DIR/<name>.npy:
      mean_loss.npy  float64 [1]  the mean training loss train_model returns over the timed steps;
      params.npy     float32 [n]  the parameters after the last step's Adam update;
      grads.npy      float32 [n]  their gradients from the last step's backward (before the clip);
    params / grads: the same fixed sample of n = 2^22 element positions (torch.randperm with a CPU generator seeded `seed`, sorted) of
    all trainable parameters concatenated in registration order (the whole set: 38 M values, 153 MB per array).  The inputs (weights,
    batches, omega and dropout draws) are seeded, so two runs with the same arguments see the same ones."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    params = [p for p in model.parameters() if p.requires_grad]
    total = sum(p.numel() for p in params)
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(total, generator=g)[:DUMP_SAMPLE].sort().values.to(params[0].device)
    with torch.no_grad():
        flat_p = torch.cat([p.detach().reshape(-1).float() for p in params])
        flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).float() for p in params])
        arrays = {'params': flat_p[idx].cpu().numpy(), 'grads': flat_g[idx].cpu().numpy()}
    arrays['mean_loss'] = np.array([mean_loss], dtype=np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)


def launch_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N ranks (one per GPU) through torch.distributed.run and exit with its
    status.  Fails instead of shrinking the job when the node has fewer than N GPUs."""
    import socket
    import subprocess
    have = torch.cuda.device_count()
    if have < n and os.environ.get('EMO_BENCH_SHARE_GPU') != '1':
        sys.exit('bench.py: --gpus %d requested but %d GPU(s) visible: refusing to run (one process per GPU, no oversubscription)' % (n, have))
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=64, help='sequences per GPU (BASELINE.md: B=64)')
    ap.add_argument('--seq', type=int, default=CFG['seq'])
    ap.add_argument('--redraw', default='every_forward')
    ap.add_argument('--dump-outputs', metavar='DIR', help="write the last timed step's outputs to DIR/<name>.npy (rank 0)")
    ap.add_argument('--full', action='store_true', help='also run the legs below (roofline, power, step0 check, gen, b4, fp32, stage1, gpt2, '
                                                        'CPU baselines); a plain run only times the training step')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-roofline', action='store_true')
    ap.add_argument('--no-gen', action='store_true')
    ap.add_argument('--no-stage1', action='store_true')
    ap.add_argument('--no-gpt2', action='store_true')
    ap.add_argument('--no-step0-check', action='store_true')
    ap.add_argument('--no-b4', action='store_true')
    ap.add_argument('--no-fp32', action='store_true', help='skip the fp32 parity-mode leg')
    ap.add_argument('--dp-selftest', action='store_true', help='N > 1: run only the gradient-exchange self-test and exit')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')

    want = max(args.gpus, 1)
    if 'WORLD_SIZE' not in os.environ and want > 1:
        launch_ranks(want)                                   # never returns
    from emo_disentanger_amd import dp, ops
    from emo_disentanger_amd.data import synthetic_batch
    from emo_disentanger_amd.model.music_performer import MusicPerformer
    from emo_disentanger_amd.optim import FusedAdam
    rank, local_rank, world = dp.env_world()
    if world != want:
        sys.exit('bench.py: --gpus %d but WORLD_SIZE=%d: launch with `python bench.py --gpus %d` (it starts the ranks itself) or '
                 '`python -m torch.distributed.run --nproc-per-node %d ... bench.py --gpus %d`' % (want, world, want, want, want))
    share = os.environ.get('EMO_BENCH_SHARE_GPU') == '1'     # TEST ONLY: several ranks on one GPU (host-staged gloo plane) to exercise the N > 1 code path
    if torch.cuda.device_count() < (local_rank + 1 if world > 1 else 1) and not share:
        sys.exit('bench.py: rank %d needs GPU %d but only %d visible: one process per GPU, no sharing' % (rank, local_rank, torch.cuda.device_count()))
    dp.init_distributed(strict=True)                         # the N > 1 line measures emo_comm_* (RCCL behind the C-ABI) or fails
    local_dev = (local_rank % max(torch.cuda.device_count(), 1)) if world > 1 else 0
    torch.cuda.set_device(local_dev)
    dev = torch.device('cuda', local_dev)
    torch.manual_seed(0)
    B, T = args.batch, args.seq
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):             # the constructor prints '[info] model init completed' like the reference's; stdout carries ONE JSON line
        model = MusicPerformer(CFG['n_token'], CFG['n_layer'], CFG['n_head'], CFG['d_model'], CFG['d_ff'], CFG['d_model'],
                               favor_feature_dims=CFG['n_feat'], use_segment_emb=True, n_segment_types=2, dropout=0.1,
                               compute_dtype='bf16', redraw=args.redraw).to(dev)
    model.train()
    selftest = None
    if world > 1:
        if dp.data_plane() != 'rccl' and os.environ.get('EMO_COMM') is None:
            sys.exit('bench.py: data plane is %r, expected the C-ABI RCCL plane' % dp.data_plane())
        if dp.data_plane() == 'rccl' and ops.lib.emo_comm_world() != want:
            sys.exit('bench.py: emo_comm_world() = %d but --gpus %d' % (ops.lib.emo_comm_world(), want))
        dp.sync_model_from_rank0(model)
        selftest = dp_selftest(model, rank, world)
        if not selftest['ok']:
            sys.exit('bench.py: data-parallel self-test failed on rank %d: %s' % (rank, selftest))
        if args.dp_selftest:
            if rank == 0:
                print(json.dumps({'dp_selftest': selftest, 'n_gpus': world, 'comm': dp.data_plane()}), flush=True)
            dp.barrier()
            dp.shutdown()
            return
    max_lr, eta_min, warmup_steps, T_max = 1e-4, 1e-5, 200, 500000      # pop1k7_pretrain.yaml
    opt = FusedAdam(model, lr=max_lr, max_grad_norm=0.5, world_size=world, token_weighted=True)
    batches = [synthetic_batch(CFG['n_token'], B, T, seed=dp.shard_seed(1234, rank) + 100 * i, device=dev) for i in range(2)]
    for b in batches:                                        # non-pad target count of the rank's batch (token-weighted DP mean)
        b['n_tok'] = (b['dec_target'] != CFG['n_token'] - 1).sum().to(torch.float32)
    s0 = step0_check(model, batches[1]) if (args.full and world == 1 and not args.no_step0_check) else None     # batches[1] = the batch of step 1
    # The timed step IS the product loop: train.train_model (zero_grad, forward with the omega redraw, loss, backward with the
    # overlapped gradient exchange at N > 1, clip(0.5) + Adam fused, LR schedule, loss bookkeeping on the device) over K synthetic
    # batches that are already resident in HBM, verbose off (= no per-step host sync; the reference's per-step print would add one).
    import tempfile
    from emo_disentanger_amd import train as tr
    tcfg = tr.TrainConfig(warmup_steps=warmup_steps, max_lr=max_lr, min_lr=eta_min, lr_decay_steps=T_max, redraw_prob=1.0, log_interval=10 ** 9,
                          ckpt_dir=tempfile.mkdtemp(prefix='emo_bench_'), world_size=world, verbose=False)
    pad = CFG['n_token'] - 1

    class Loader:
        """n synthetic batches; a HIP event is recorded on the compute stream every time the loop fetches a batch (= step boundaries)."""

        def __init__(self, n, record=False):
            self.n, self.events = n, [] if record else None

        def __len__(self):
            return self.n

        def __iter__(self):
            for i in range(self.n):
                if self.events is not None:
                    e = torch.cuda.Event(enable_timing=True)
                    e.record()
                    self.events.append(e)
                yield batches[i % len(batches)]

    def run_steps(n, record=False):
        ld = Loader(n, record)
        loss = tr.train_model(1, model, ld, opt, None, pad, model_type='performer', cfg=tcfg)
        return loss, ld.events

    def step():
        run_steps(1)

    if args.warmup > 0:
        run_steps(args.warmup)
    torch.cuda.synchronize()
    dp.barrier()
    sampler = PowerSampler() if (args.full and rank == 0) else None
    if sampler is not None:
        sampler.start()
    t0 = time.perf_counter()
    mean_loss, evs = run_steps(args.steps, record=True)
    end_ev = torch.cuda.Event(enable_timing=True)
    end_ev.record()
    torch.cuda.synchronize()
    dp.barrier()
    my_elapsed = time.perf_counter() - t0
    power = sampler.result() if sampler is not None else None
    elapsed = dp.max_over_ranks(my_elapsed)
    per_step = [a.elapsed_time(b_) for a, b_ in zip(evs, evs[1:] + [end_ev])]       # ms, device timeline of this rank
    median_ms = sorted(per_step)[len(per_step) // 2] if per_step else float('nan')
    tokens = world * B * T * args.steps
    value = tokens / elapsed
    out = {'metric': 'train tokens/sec (+ AR gen tokens/sec in "gen"), stage2 Performer d512 L12 seq%d' % T, 'value': round(value, 1), 'unit': 'tokens/s', 'n_gpus': world,
           'rccl_ranks': (ops.lib.emo_comm_world() if dp.data_plane() == 'rccl' else world if dp.data_plane() == 'nccl' else 0), 'comm': dp.data_plane() or 'none',
           'steps': args.steps, 'steps_timed': len(per_step), 'warmup': args.warmup, 'ms_per_step': round(1000 * elapsed / args.steps, 3), 'higher_is_better': True,
           'scaling': 'weak', 'vs_baseline': None, 'dtype': 'bf16', 'data': 'synthetic',
           'config': {'workload': 'BASELINE configs[%d]: stage2 Performer d_model=512 n_layer=12 n_head=8 favor_dims=128 seq=%d, B=%d/GPU, '
                                  'dropout 0.1, omega redraw %s, fwd+bwd+allreduce+clip+Adam' % (1 if world == 1 else 2, T, B, args.redraw),
                      'global_batch': world * B, 'seq_len': T, 'parallelism': 'dp%d' % world, 'n_token': CFG['n_token']},
           'mean_loss': round(mean_loss, 4), 'gemm_tflops_model': round(value * gemm_flops_per_token() / 1e12, 1),
           'timed_loop': 'emo_disentanger_amd.train.train_model (the product loop), verbose off',
           'median_ms_per_step': round(median_ms, 3), 'median_tokens_per_s': round(world * B * T / (median_ms / 1e3), 1) if median_ms == median_ms else None,
           'power': power}
    if args.dump_outputs and rank == 0:      # before the roofline's instrumented steps change the weights
        dump_outputs(model, mean_loss, args.dump_outputs)
    if args.full and not args.no_roofline:   # every rank runs the instrumented steps (they contain the all-reduce)
        roof = dominant_kernel_roofline(step, B, T)
        if rank == 0:
            out['roofline'] = roof
    if world > 1:
        # per-rank view of the timed region + the exchange measured by the self-test (HIP events, communication stream included)
        allt = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        import torch.distributed as dist
        dist.all_gather(allt, torch.tensor([my_elapsed / args.steps * 1e3], dtype=torch.float64))
        out['per_rank_ms_per_step'] = [round(float(t), 3) for t in allt]
        out['dp_selftest'] = selftest
    if rank == 0:
        if s0 is not None:
            out['step0_check'] = s0
        legs = args.full and world == 1
        if legs and not args.no_gen:
            out['gen'] = generation_bench(model)
            if not args.no_cpu_baseline:
                out['gen']['cpu_baseline'] = cpu_generation_baseline()
        if legs and not args.no_b4:
            out['b4'] = b4_bench(model, FusedAdam, tr)
        if legs and not args.no_fp32:
            out['fp32_parity'] = fp32_parity_bench(tr, FusedAdam, B, T)
            torch.cuda.empty_cache()
        if legs and not args.no_stage1:
            out['stage1'] = stage1_bench()
        if legs and not args.no_gpt2:
            del model, opt                                   # (the Performer's 21 GB of saved activations are not needed any more)
            torch.cuda.empty_cache()
            out['gpt2'] = gpt2_bench()
            if not args.no_gen:
                torch.cuda.empty_cache()
                out['gen_gpt2'] = gpt2_generation_bench()
        if legs and not args.no_cpu_baseline:
            out['cpu_baseline'] = cpu_baseline(min(T, 2048))
        print(json.dumps(out), flush=True)
    if world > 1:
        dp.barrier()
        dp.shutdown()


if __name__ == '__main__':
    main()
