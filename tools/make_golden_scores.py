#!/usr/bin/env python3
"""Generate tests/golden/score_gpt2_tiny.npz by IMPORTING the real reference (same recipe and the same constraints as
tools/make_golden.py: runs only where the reference checkout is present, the fixture holds numbers only — inputs, targets and the
reference's own compute_loss(reduction='none' / 'sum' / 'mean') values; weights are regenerated from the seed by oracle/weights.py).
Usage: PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_scores.py"""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, install_reference  # noqa: E402

CASE = dict(V=327, L=2, H=4, d=64, dff=256, T=96, B=3, scale=4.0, seed=21)


def main():
    install_reference()
    from model.music_gpt2 import MusicGPT2
    from oracle.weights import make_state_dict
    c = CASE
    sd = make_state_dict('gpt2', c['V'], c['L'], c['H'], c['d'], c['dff'], n_segment_types=2, seed=c['seed'], scale=c['scale'])
    model = MusicGPT2(c['V'], c['L'], c['H'], c['d'], c['dff'], c['d'], dropout=0.0, use_segment_emb=True, n_segment_types=2)
    model.load_state_dict(sd)
    model.eval()
    rng = np.random.default_rng(2000 + c['seed'])
    x = torch.from_numpy(rng.integers(0, c['V'] - 1, size=(c['B'], c['T']), dtype=np.int64))
    seg = torch.from_numpy((np.arange(c['T'])[None, :] // 12 % 2).repeat(c['B'], 0).astype(np.int64))
    tgt = torch.from_numpy(rng.integers(0, c['V'] - 1, size=(c['B'], c['T']), dtype=np.int64))
    tgt[seg == 0] = c['V'] - 1                      # the lead-sheet spans are pad targets, as in the dataset
    with torch.no_grad():
        logits = model(x, seg_inp=seg)
        out = {r: model.compute_loss(logits, tgt, reduction=r)['recons_loss'] for r in ('none', 'sum', 'mean')}
    assert out['none'].shape == (c['B'] * c['T'],)
    np.savez_compressed(os.path.join(OUT, 'score_gpt2_tiny.npz'), x=x.numpy(), seg=seg.numpy(), tgt=tgt.numpy(),
                        nll_none=out['none'].numpy(), nll_sum=np.float32(out['sum'].item()), nll_mean=np.float32(out['mean'].item()),
                        cfg_keys=np.array(sorted(c)), cfg_vals=np.array([float(c[k]) for k in sorted(c)]))
    print('[golden] score_gpt2_tiny: mean', out['mean'].item(), 'sum', out['sum'].item())


if __name__ == '__main__':
    main()
