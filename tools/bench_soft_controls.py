"""What the soft sampling controls cost in the grammar launch (emo_grammar_step: tok_bias / n_biases / bias_of / top_k_of / min_p_of).
The ACC, ACC_WINDOW (2048-token window) and TXL launches of bench_sampling_controls.py (its rig: 32 streams, V = 327 / 327 / 200, randn x 3
logits, every stream drawing in every launch), in three cases:
  (a) null      every new field NULL;
  (b) controls  all three on: four bias rows (randn x 2, the likely PAD at -inf) shared by the 32 streams, top_k 8 .. 39 and min_p
                0.005 .. 0.05 per stream;
  (c) parent    the library of the parent commit (--parent-lib PATH: a libemo_hip.so built from the commit before this feature, driven through
                a ctypes mirror of ITS shorter block, the current one without the five fields) on the launch of (a).  Left out without the flag.
The cases run the same number of launches from the same start state, alternating a, c, b in every repeat; a figure is the median over the
repeats of the mean launch time of a back-to-back batch, and its spread the min / max over the repeats.  Writes
profiles/soft_controls_bench.json and prints it as one JSON line.  No pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_sampling_controls as bsc  # noqa: E402

N = bsc.N
bsc.NEW = ('tok_bias', 'n_biases', 'bias_of', 'top_k_of', 'min_p_of')       # (ParentLib: the parent's block is the current one without the five)


def controls(V):
    """-> (0 ban rows, the tables of the three soft controls and n_biases, as block_set takes them)."""
    from emo_disentanger_amd import gen_loop
    rs = np.random.RandomState(1)
    rows = (rs.randn(4, V) * 2).astype(np.float32)
    rows[:, V - 1] = -np.inf
    ctl = gen_loop.draw_controls('bench', N, V, bias=[rows[r % 4] for r in range(N)], top_k=[8 + r for r in range(N)],
                                 min_p=np.linspace(0.005, 0.05, N).tolist())
    tabs = ctl.tables()
    out = {k: torch.from_numpy(v).cuda() for k, v in tabs.items()}
    out['n_biases'] = len(tabs['tok_bias'])
    return 0, out


bsc.controls = controls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--parent-lib', default=None, help='libemo_hip.so of the commit before the soft controls: case (c)')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'soft_controls_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import ops
    torch.cuda.set_device(0)
    parent = bsc.ParentLib(args.parent_lib) if args.parent_lib else None
    cases = ['null'] + (['parent'] if parent else []) + ['controls']
    out = {'tool': 'bench_soft_controls', 'device': torch.cuda.get_device_name(0), 'runs': 'one run on one machine', 'streams': N,
           'launches': args.launches, 'repeats': args.repeats, 'parent_lib': bool(parent), 'launch': {}}
    for kind in (bsc.ACC, bsc.WIN, bsc.TXL):
        us = {c: [] for c in cases}
        seqs = {}
        for _ in range(args.repeats):
            for c in cases:
                x, acc, seq = bsc.time_case(ops, kind, c, args.launches, args.warmup, parent)
                us[c].append(x)
                seqs[c] = (acc, seq)
        if parent:                                               # the same draws from the same start: the launch of (a) is the parent's
            assert seqs['null'][0] == seqs['parent'][0] and torch.equal(seqs['null'][1], seqs['parent'][1])
        assert not torch.equal(seqs['null'][1], seqs['controls'][1])         # ... and the controls bite
        rec = {'V': 200 if kind == bsc.TXL else 327}
        for c in cases:
            rec['us_' + c] = round(statistics.median(us[c]), 2)
            rec['us_%s_min_max' % c] = [round(min(us[c]), 2), round(max(us[c]), 2)]
        rec['us_controls_minus_null'] = round(rec['us_controls'] - rec['us_null'], 2)
        if parent:
            rec['us_null_minus_parent'] = round(rec['us_null'] - rec['us_parent'], 2)
            rec['us_spread_null'] = round(max(us['null']) - min(us['null']), 2)
            rec['us_spread_parent'] = round(max(us['parent']) - min(us['parent']), 2)
        out['launch'][bsc.NAMES[kind]] = rec
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
