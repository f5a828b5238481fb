"""What the per-job sampling controls cost in the grammar launch (emo_grammar_step: tok_mask / mask_of / temp_of / top_p_of).
The ACC, ACC_WINDOW (2048-token window) and TXL launches at the shapes of bench_draw_scores.py: 32 streams, V = 327 / 327 / 200, randn x 3
logits, every stream drawing in every launch, in three cases:
  (a) null      every new field NULL;
  (b) controls  four ban rows (a tenth of the vocabulary each, never the likely tokens' row twice) shared by the 32 streams, and per-stream
                temp_of / top_p_of;
  (c) parent    the library of the parent commit (--parent-lib PATH: a libemo_hip.so built from the commit before this feature, driven through
                a ctypes mirror of ITS block, the one without the new fields) on the launch of (a).  Left out without the flag.
The cases run the same number of launches from the same start state, alternating a, c, b in every repeat; a figure is the median over the
repeats of the mean launch time of a back-to-back batch, and its spread the min / max over the repeats.  Writes
profiles/sampling_controls_bench.json and prints it as one JSON line.  No pass / fail threshold."""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import torch  # noqa: E402

TXL, ACC, WIN = 0, 1, 2
NAMES = {TXL: 'txl', ACC: 'acc', WIN: 'acc_window'}
N = 32
NEW = ('tok_mask', 'n_masks', 'mask_of', 'temp_of', 'top_p_of')


def rig(kind, launches, seed=0):
    """32 streams that draw in every launch (every event plain but PAD, which is banned or all but never drawn) -> (numbers, tensors)."""
    V = 200 if kind == TXL else 327
    W = 2048
    L = W if kind == WIN else 3
    width = L + launches + 8
    dev = 'cuda'
    g = torch.Generator(device=dev).manual_seed(seed)
    flags = torch.zeros(V, dtype=torch.int32, device=dev)
    flags[V - 1] = 4
    params, state = torch.zeros(N, 8, dtype=torch.int32, device=dev), torch.zeros(N, 8, dtype=torch.int32, device=dev)
    state[:, 1] = L
    if kind == TXL:
        params[:, 0], params[:, 1], params[:, 2], state[:, 6] = 1 << 20, 1 << 20, L, L
    else:
        params[:, 0], params[:, 1], params[:, 4], state[:, 2] = 1 << 20, 1 << 20, 1, L
    logits = (torch.randn(N, V, device=dev, generator=g) * 3).contiguous()
    logits[:, V - 1] = -30.0
    t = dict(logits=logits, u_steps=torch.rand(4 * launches, N, device=dev, generator=g),
             ev_flags=flags, ev_beat=torch.zeros(V, dtype=torch.int32, device=dev), params=params, state=state,
             seq=torch.zeros(N, width, dtype=torch.int64, device=dev), running=torch.tensor([N], dtype=torch.int32, device=dev))
    num = dict(n_rows=N, n_token=V, ld_u=N, temperature=1.2, top_p=0.9)
    if kind == TXL:
        num.update(key_temperature=1.1, key_top_p=0.97)
        t.update(tok_out=torch.zeros(N, dtype=torch.int64, device=dev))
    else:
        t.update(segs=torch.zeros(N, width, dtype=torch.int64, device=dev), lead_tok=torch.zeros(4, dtype=torch.int64, device=dev),
                 lead_off=torch.tensor([0, 2, 4], dtype=torch.int32, device=dev))
        if kind == ACC:
            num.update(max_len=width + 8, pad=V - 1)
            t.update(tok_out=torch.zeros(N, dtype=torch.int64, device=dev), seg_out=torch.zeros(N, dtype=torch.int64, device=dev))
        else:
            num.update(window=W)
            t.update(win_tok=torch.zeros(N, W, dtype=torch.int64, device=dev), win_seg=torch.zeros(N, W, dtype=torch.int64, device=dev))
    return num, t


def controls(V):
    """Four ban rows of V // 10 ids each (PAD among them) for the 32 streams, per-stream temperatures 1.0 .. 1.4 and top_p 0.85 .. 0.97."""
    from emo_disentanger_amd import gen_loop
    rs = np.random.RandomState(1)
    bans = [sorted(set(rs.choice(V - 1, size=V // 10, replace=False).tolist()) | {V - 1}) for _ in range(4)]
    ctl = gen_loop.draw_controls('bench', N, V, [bans[r % 4] for r in range(N)], np.linspace(1.0, 1.4, N).tolist(), np.linspace(0.85, 0.97, N).tolist())
    tabs = ctl.tables()
    n_masks = len(tabs['tok_mask'])
    tabs['tok_mask'] = tabs['tok_mask'].view(np.int32)
    return n_masks, {k: torch.from_numpy(v).cuda() for k, v in tabs.items()}


class ParentLib:
    """The parent commit's library behind the mirror of its own block: the current mirror without the new fields."""

    def __init__(self, path):
        from emo_disentanger_amd import _lib
        self.lib = ctypes.CDLL(path)

        class Step(ctypes.Structure):
            _fields_ = [f for f in _lib.GrammarStep._fields_ if f[0] not in NEW]

        self.Step = Step
        self.lib.emo_grammar_step_size.restype = ctypes.c_int
        size = self.lib.emo_grammar_step_size()
        if size != ctypes.sizeof(Step):
            raise SystemExit('%s: its emo_grammar_step_t has %d bytes, the block without the new fields %d: not the parent commit\'s library'
                             % (path, size, ctypes.sizeof(Step)))
        self.lib.emo_grammar_step.restype = ctypes.c_int
        self.lib.emo_grammar_step.argtypes = [ctypes.POINTER(Step), ctypes.c_void_p]
        self.lib.emo_last_error.restype = ctypes.c_char_p
        self.stream = _lib.stream

    def block(self, kind, num, t):
        a = self.Step(kind=kind, ld_seq=t['seq'].shape[1], n_u=t['u_steps'].shape[0], **num)
        for k, v in t.items():
            setattr(a, k, v.data_ptr())
        return a

    def step(self, a):
        if self.lib.emo_grammar_step(ctypes.byref(a), self.stream()) != 0:
            raise SystemExit('parent library: ' + self.lib.emo_last_error().decode())


def time_case(ops, kind, case, launches, warmup, parent):
    num, t = rig(kind, launches + warmup)
    if case == 'parent':
        args = parent.block(kind, num, t)
        step = lambda: parent.step(args)                         # noqa: E731
    else:
        held = {}
        args = ops.GrammarStep(kind=kind)
        ops.block_set(args, held, **num, **t)
        if case == 'controls':
            n_masks, tabs = controls(num['n_token'])
            ops.block_set(args, held, n_masks=n_masks, **tabs)
        step = lambda: ops.grammar_step(args)                    # noqa: E731
    for _ in range(warmup):
        step()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(launches):
        step()
    b.record()
    torch.cuda.synchronize()
    assert int(t['running'].item()) == N, 'a stream left RUNNING: the launches timed are not all drawing launches'
    accepted = int(t['state'][:, 2 if kind == TXL else 7].sum().item())
    return 1e3 * a.elapsed_time(b) / launches, accepted, t['seq'].clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--parent-lib', default=None, help='libemo_hip.so of the commit before the sampling controls: case (c)')
    ap.add_argument('-o', '--output', default=os.path.join(os.path.dirname(HERE), 'profiles', 'sampling_controls_bench.json'))
    args = ap.parse_args()
    from emo_disentanger_amd import ops
    torch.cuda.set_device(0)
    parent = ParentLib(args.parent_lib) if args.parent_lib else None
    cases = ['null'] + (['parent'] if parent else []) + ['controls']
    out = {'tool': 'bench_sampling_controls', 'device': torch.cuda.get_device_name(0), 'streams': N, 'launches': args.launches,
           'repeats': args.repeats, 'parent_lib': bool(parent), 'launch': {}}
    for kind in (ACC, WIN, TXL):
        us = {c: [] for c in cases}
        seqs = {}
        for _ in range(args.repeats):
            for c in cases:
                x, acc, seq = time_case(ops, kind, c, args.launches, args.warmup, parent)
                us[c].append(x)
                seqs[c] = (acc, seq)
        if parent:                                               # the same draws from the same start: the launch of (a) is the parent's
            assert seqs['null'][0] == seqs['parent'][0] and torch.equal(seqs['null'][1], seqs['parent'][1])
        rec = {'V': 200 if kind == TXL else 327}
        for c in cases:
            rec['us_' + c] = round(statistics.median(us[c]), 2)
            rec['us_%s_min_max' % c] = [round(min(us[c]), 2), round(max(us[c]), 2)]
        rec['us_controls_minus_null'] = round(rec['us_controls'] - rec['us_null'], 2)
        if parent:
            rec['us_null_minus_parent'] = round(rec['us_null'] - rec['us_parent'], 2)
            rec['us_spread_null'] = round(max(us['null']) - min(us['null']), 2)
            rec['us_spread_parent'] = round(max(us['parent']) - min(us['parent']), 2)
        out['launch'][NAMES[kind]] = rec
    os.makedirs(os.path.dirname(args.output), exist_ok=True)
    with open(args.output, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
