"""bench.py's own contract: `--steps` sets the timed steps, a plain run carries only the headline legs, and `--dump-outputs`
writes the last timed step's outputs, from the same inputs in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_a_fixed_sample_of_parameters_and_gradients(tmp_path):
    # every parameter element holds its own position in the concatenation (exact in fp32 below 2^24), its gradient minus that: the dumped
    # arrays then name the sampled positions themselves, which are pinned here by value
    m = torch.nn.Sequential(torch.nn.Linear(3000, 1500), torch.nn.Linear(1500, 7))
    off = 0
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.arange(off, off + p.numel(), dtype=torch.float32).view_as(p))
            p.grad = -p.detach().clone()
            off += p.numel()
    assert off == 4512007 and off > bench.DUMP_SAMPLE
    for d in ('a', 'b'):
        bench.dump_outputs(m, 5.25, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['grads.npy', 'mean_loss.npy', 'params.npy']
    a = {n: np.load(tmp_path / 'a' / n) for n in names}
    assert a['params.npy'].dtype == np.float32 and a['grads.npy'].dtype == np.float32
    assert a['mean_loss.npy'].dtype == np.float64 and a['mean_loss.npy'].tolist() == [5.25]
    pos = a['params.npy'].astype(np.int64)
    assert pos.shape == (bench.DUMP_SAMPLE,) and (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < off
    np.testing.assert_array_equal(a['grads.npy'], -a['params.npy'])
    left_out = np.setdiff1d(np.arange(off), pos)
    assert len(left_out) == 317703 and left_out[:6].tolist() == [52, 81, 102, 136, 143, 162] and int(left_out.sum()) == 716612359914
    for n in names:
        np.testing.assert_array_equal(a[n], np.load(tmp_path / 'b' / n))
    assert sum(os.path.getsize(tmp_path / 'a' / n) for n in names) <= 64 << 20


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--steps' in r.stderr and '"value"' not in r.stdout


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_asked_and_dumps_reproducible_outputs(tmp_path):
    lines, dumps = [], []
    for i in range(2):
        d = str(tmp_path / ('run%d' % i))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4',
                            '--dump-outputs', d], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [l for l in r.stdout.splitlines() if l.startswith('{')]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
        dumps.append({n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))})
    for ln in lines:
        assert ln['steps'] == ln['steps_timed'] == 3 and ln['warmup'] == 1       # steps_timed: step-boundary events the timed loop recorded
        assert ln['ms_per_step'] > 0 and ln['unit'] == 'tokens/s' and ln['dtype'] == 'bf16' and ln['higher_is_better'] is True
        assert not {'roofline', 'step0_check', 'gen', 'b4', 'fp32_parity', 'stage1', 'gpt2', 'cpu_baseline'} & set(ln)
    assert sorted(dumps[0]) == ['grads.npy', 'mean_loss.npy', 'params.npy']
    assert np.isfinite(dumps[0]['grads.npy']).all() and np.abs(dumps[0]['grads.npy']).max() > 0
    assert abs(float(dumps[0]['mean_loss.npy'][0]) - lines[0]['mean_loss']) <= 1e-4
    # Same arguments => same inputs.  The step is reproducible to bf16 rounding only: the backward accumulates with atomics, and an fp32 sum
    # that lands on the other side of a bf16 rounding boundary changes that activation by 2^-8 downstream.  Measured on the MI355X at this
    # shape, 7 pairs of runs: |dloss| <= 2.3e-6, max |dgrad| <= 2.8e-3 of max |g|, at most 4 of the 4.2 M parameters > 1e-6 apart.
    a, b = dumps
    assert abs(float(a['mean_loss.npy'][0]) - float(b['mean_loss.npy'][0])) <= 2e-5
    # Adam divides by |g|: where a gradient element is near zero its sign can flip between runs, which moves that parameter's update from
    # +lr to -lr.  Step 1 runs at the optimizer's initial lr = 1e-4 (train_model writes the warm-up lr = 1e-4 k / 200 only after step k),
    # steps 2-4 at 5e-7, 1e-6, 1.5e-6; over four steps Adam's |m_hat| / sqrt(v_hat) stays below 1.01 (Cauchy-Schwarz on its weights), so no
    # element can move further apart than the bound below.
    lrs = [1e-4] + [1e-4 * k / 200 for k in (1, 2, 3)]
    d = np.abs(a['params.npy'].astype(np.float64) - b['params.npy'])
    assert d.max() <= 2 * 1.01 * sum(lrs) + 1e-6, d.max()
    assert (d > 1e-6).mean() <= 1e-4, ((d > 1e-6).sum(), d.size)          # only the rare near-zero gradient elements
    assert np.abs(a['grads.npy'] - b['grads.npy']).max() <= 1e-2 * np.abs(a['grads.npy']).max()
