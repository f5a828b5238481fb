"""Every emo_gemm route against the EXACT integer oracle (tests/gemm_exact_ref.py), the route asserted first.

Operands are small integers (A, B in [-3, 3]; bias in [-8, 8]; residual / mul_aux / accumulate base in [-64, 64]; mul_scale = 2; p_drop = 0.5, whose
multiplier is exactly 2), so every fp32 accumulation is exact in any order: an fp32 output must EQUAL the integer result and a bf16 output its one
round-to-nearest-even conversion, whichever kernel, ring geometry or K-split ran.  Every case asserts, in this order: the kernel family
(emo_gemm_last_kernel() & 15), the split-K flags (+ 16 workspace, + 32 reduce-and-epilogue pass), the plan fields it names
(emo_gemm_last_plan(): BK | stages << 8 | splits << 16 | column split << 24), then torch.equal for every output.  The split-K workspace of every
case is an exactly-sized buffer between two guard bands that must stay untouched.

bf16-output cases assert that their own reference has outputs above 256 (where a bf16 accumulator or a double rounding would show).  Below
K = 512, and on outputs too small to have such values by chance, BOTH operands are shifted to [0, 6]: shifting one leaves the products' mean at
zero, and at K = 32 nothing would reach 256.

Routes and edges, per family:
  5  LDS-DMA ring: small grids (<= 512 blocks) on the 4-stage ring — BK 32 at K = 128 (K-tiles = stages) and 160, BK 64 at K = 512 and 576; large
     grids (> 512 blocks: 129 x 8328, whose single row of tiles is rounded up to 8, and 8328 x 1024) on BK32x3 at K = 32 / 64 / 96 / 128 (1 - 4
     tiles on a 3-stage ring), BK32x2 at K = 32 / 64 (NN), BK64x2 at K = 1088; layouts NT, NN and (variant 3, K <= 4096) TN, TT; edge tiles at
     M in {8, 129} x N in {8, 327}; padded row strides; a strided output view inside a guard value.
  6  register-staged: K % 32 != 0 (37, 264) in all four layouts, M < 8, N < 8, and EMO_GEMM_SAFE_TR=1 in a child process (the switch is latched).
  split-K: plain fp32 wgrad through the workspace (+ 16) and through atomics with 2 / 4 / 8 and the odd counts 3 / 5 (ragged last split),
     accumulate onto an integer base; the reduce-and-epilogue pass (+ 32) at 128 x 128 x 1024 and at 2048 x 512 x 2048 with the full epilogue.
  1  skinny: M in {1, 17, 32} x N in {8, 24, 327} x K in {32, 96, 160, 512, 1024, 1056, 2048, 2080}: 4 / 8 / 16 waves, empty wave slices, partial chunks.
  2  A-stationary: M = ASTAT_MIN_ROWS and + 128, N in {64, 128, 512, 2048}, the column split from the plan (1 / 1 / 4 / 16) and forced to 2, one case
     per instantiation that is exact on integers, strided A and C views, refusals.
  4  256 x 256 NT under EMO_GEMM_W128=1: K = 4 BK, 320, 1088; plain / bias / residual / bias + dropout + residual.
  3  256 x 256 wgrad: default thresholds at 1024 x 768 x 8192 (8 splits); thresholds lowered: 1, 2, 3, 5, 6, 12 tiles, both bias-gradient layouts,
     accumulate, a workspace without room for the bias partials, a workspace too small for the product.
  7  fp32: 64- and 128-tile plans, unaligned strides, split-K with a ragged last split.

Where the dispatcher admits something else than the issue behind this file assumed:
  * the 256 x 256 wgrad plan has no `extra` splits at 3 tiles (32 / 3 = 10 full splits per XCD are capped at 8, which ends the plan at 64 splits); the
    extra branch runs at 5, 6 and 12 tiles (3 / 2 / 5 extra splits), so 5 tiles was added and 3 tiles asserts 64 splits;
  * an A operand one element off its 16-byte alignment is refused by EVERY bf16 kernel (emo_gemm raises); the A-stationary refusal that lands on
    the ring is an output row stride that is no multiple of 8 elements."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_exact_ref as X

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
LAYOUTS = {'NT': (False, False), 'NN': (False, True), 'TT': (True, False), 'TN': (True, True)}    # (a_trans, b_trans): A stored [K, M] / B stored [K, N]
GUARD = 1 << 16


def _ops():
    from emo_disentanger_amd import ops
    return ops


class _Env:
    """Environment switches for one call; the per-shape workspace-size cache of ops is dropped around them (they change the plan)."""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        _ops()._ws_need.clear()

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _ops()._ws_need.clear()
        return False


def _wide(rows, cols, lo, hi, seed, dtype, pad, zeros=0.0):
    """Integer tensor [rows, cols] as a view of a wider one (bf16 rows are 16-byte multiples; pad: further columns), on the host and on the device."""
    full = (cols + 7) // 8 * 8 + pad if dtype == BF16 else cols + pad
    h = X.ints((rows, full), lo, hi, seed, dtype, zeros)
    return h[:, :cols], h.cuda()[:, :cols]


def _run(M, N, K, fam, *, layout='NT', in_dtype=BF16, out_dtype=BF16, flags=0, plan=None, epi=(), pad=0, out_pad=0, seed=0, env=None, accumulate=False,
         rowsum=None, ws_bytes=None, shift=None, mask_out=False, bitmask=None):
    """One ops.gemm on integer operands: family, split flags, plan fields, then every output against the oracle.  epi: subset of
    {'bias', 'aux', 'relu', 'mul', 'drop', 'res'}; pad / out_pad: extra columns of the operand / output row stride; rowsum: 'a' | 'b';
    ws_bytes: workspace size offered (a function of the size the library asks for; default: exactly that size); bitmask = (device mask, host bool
    mask): EMO_MUL_BITMASK.  Returns (device output, Expected, device mask or None)."""
    ops = _ops()
    a_t, b_t = LAYOUTS[layout]
    if shift is None:        # bf16 outputs need values above 256 to see a wrong rounding (module docstring)
        shift = out_dtype == BF16 and (K < 512 or M * N < 65536)
    lo, hi = (0, 6) if shift else (-3, 3)
    Ah, Ad = _wide(*((K, M) if a_t else (M, K)), lo, hi, 1000 + seed, in_dtype, pad)
    Bh, Bd = _wide(*((K, N) if b_t else (N, K)), lo, hi, 2000 + seed, in_dtype, pad)

    def mn(lo_, hi_, s, zeros=0.0):        # an [M, N] epilogue operand with the output's row stride
        full = X.ints((M, N + out_pad), lo_, hi_, s, out_dtype, zeros)
        return full[:, :N], full.cuda()[:, :N]

    kw, ref = dict(a_trans=a_t, b_trans=b_t), dict(a_trans=a_t, b_trans=b_t, out_dtype=out_dtype)
    aux_d = None
    if 'bias' in epi:
        bh = X.ints((N,), -8, 8, 3000 + seed, F32)
        kw['bias'], ref['bias'] = bh.cuda(), bh
    if 'aux' in epi:
        aux_d = kw['aux_out'] = torch.full((M, N + out_pad), 77.0, device='cuda', dtype=out_dtype)[:, :N]
        ref['want_aux'] = True
    if 'relu' in epi:
        kw['act'], ref['relu'] = ops.ACT_RELU, True
    if 'mul' in epi:
        mh, md = mn(-64, 64, 4000 + seed, zeros=0.4)
        kw.update(mul_aux=md, mul_mode=ops.MUL_NONZERO, mul_scale=2.0)
        ref.update(mul_aux=mh, mul_scale=2.0)
    if bitmask is not None:
        kw.update(mul_aux=bitmask[0], mul_mode=ops.MUL_BITMASK, mul_scale=2.0)
        ref.update(mul_aux=torch.from_numpy(bitmask[1].astype(np.float32)), mul_scale=2.0)
    if 'drop' in epi:
        kw.update(p_drop=0.5, seed=11, offset=3)
        ref.update(p_drop=0.5, seed=11, offset=3)
    if 'res' in epi:
        rh, rd = mn(-64, 64, 5000 + seed)
        kw['residual'], ref['residual'] = rd, rh
    outbuf = torch.full((M, N + out_pad), 77.0, device='cuda', dtype=out_dtype)
    if accumulate:
        ch, cd = mn(-64, 64, 6000 + seed)
        outbuf[:, :N] = cd
        kw['accumulate'], ref['accumulate_base'] = True, ch
    kw['out'] = outbuf[:, :N]
    rs_d = None
    if rowsum:
        rs_h = X.ints((M if rowsum == 'a' else N,), -64, 64, 7000 + seed, F32)
        rs_d = kw[rowsum + '_rowsum'] = rs_h.cuda()
        ref['want_%s_rowsum' % rowsum] = rs_h
    mask_d = None
    if mask_out:
        mask_d = kw['mask_out'] = torch.zeros(M, N // 8, device='cuda', dtype=torch.uint8)
        ref['want_mask'] = True

    held = {}

    def guarded_workspace(kind, device, need, st=None):       # exactly the bytes asked for (or ws_bytes(need)), between two guard bands
        size = need if ws_bytes is None else ws_bytes(need)
        if size <= 0:
            return None, 0
        held['buf'] = torch.full((2 * GUARD + size,), 0x5A, dtype=torch.uint8, device=device)
        held['size'] = size
        return held['buf'][GUARD:GUARD + size], size

    real_workspace, real_gemm, routed = ops._workspace, ops.lib.emo_gemm, []

    def routed_gemm(*a):                   # the route query for the very arguments of the launch, asked first
        words = ctypes.c_int(-1), ctypes.c_int(-1)
        assert ops.lib.emo_gemm_route(*a[:-1], ctypes.byref(words[0]), ctypes.byref(words[1])) == 0, ops.lib.emo_last_error()
        routed.append((words[0].value, words[1].value))
        return real_gemm(*a)

    with _Env(env):
        ops._workspace, ops.lib.emo_gemm = guarded_workspace, routed_gemm
        try:
            out = ops.gemm(Ad, Bd, **kw)
            code, p = ops.lib.emo_gemm_last_kernel(), ops.lib.emo_gemm_last_plan()
        finally:
            ops._workspace, ops.lib.emo_gemm = real_workspace, real_gemm
    torch.cuda.synchronize()
    what = (M, N, K, layout, sorted(epi), env)
    # 1. the route, and the route query (which launches nothing) saying the same
    assert routed == [(code, p)], (routed, code, p, what)
    assert (code & 15) in (fam if isinstance(fam, tuple) else (fam,)), ('family %d' % (code & 15), what)
    assert (code & 48) == flags, ('split flags %d' % (code & 48), what)
    # 2. the plan fields the case names
    got_plan = dict(bk=p & 255, stages=(p >> 8) & 255, splits=(p >> 16) & 255, col=(p >> 24) & 255)
    for k, v in (plan or {}).items():
        assert got_plan[k] == v, (k, got_plan, what)
    # 3. the values
    exp = X.expected(Ah, Bh, **ref)
    if out_dtype == BF16:
        assert int(np.abs(exp.exact).max()) > 256, what
    assert out.dtype == out_dtype and torch.equal(out.cpu(), exp.out), (what, _diff(out, exp.out))
    if out_pad:
        assert bool((outbuf[:, N:] == 77.0).all()), ('wrote outside the output view', what)
    if aux_d is not None:
        assert torch.equal(aux_d.cpu(), exp.aux_out), ('aux_out', what, _diff(aux_d, exp.aux_out))
    if rs_d is not None:
        want = exp.a_rowsum if rowsum == 'a' else exp.b_rowsum
        assert torch.equal(rs_d.cpu(), want), (rowsum + '_rowsum', what, _diff(rs_d, want))
    if mask_d is not None:
        assert torch.equal(ops.bitmask_rows(mask_d, M, N).cpu(), X.pack_rows(exp.mask)), ('mask_out', what)
    if 'buf' in held:
        b, size = held['buf'], held['size']
        assert bool((b[:GUARD] == 0x5A).all()) and bool((b[GUARD + size:] == 0x5A).all()), ('workspace overrun', what)
    return out, exp, mask_d


def _diff(got, want):
    d = (got.detach().cpu().double() - want.double()).abs()
    return '%d of %d differ, max |diff| %g' % (int((d != 0).sum()), d.numel(), float(d.max()))


# ------------------------------------------------------------------------------------------- 5: the LDS-DMA ring
@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN', 'TT'])
@pytest.mark.parametrize('K,bk', [(128, 32), (160, 32), (512, 64), (576, 64)])
def test_ring_small_grid_four_stages(layout, K, bk):
    """200 x 136 (2 x 2 ragged tiles, 16 blocks): the 4-stage ring, 32-deep below K = 512 (K = 128: as many K-tiles as stages), 64-deep from there."""
    plan = dict(bk=bk, stages=4, splits=0)
    _run(200, 136, K, 5, layout=layout, plan=plan)
    _run(200, 136, K, 5, layout=layout, plan=plan, out_dtype=F32, epi=('bias', 'res'), seed=1)


@pytest.mark.parametrize('K', [32, 64, 96, 128])
def test_ring_large_grid_three_stages_with_fewer_tiles_than_stages(K):
    """More than 512 blocks, NT, K <= 1024: BK32x3 with 1, 2, 3 and 4 K-tiles (the prologue's `s < nk`, the `newer` wait selection at the tail)."""
    plan = dict(bk=32, stages=3, splits=0)
    _run(129, 8328, K, 5, plan=plan)
    _run(129, 8328, K, 5, plan=plan, out_dtype=F32, epi=('bias', 'relu', 'res'), seed=1)
    if K == 64:
        _run(8328, 1024, K, 5, plan=plan, out_dtype=F32, epi=('bias',), seed=2)


@pytest.mark.parametrize('K', [32, 64])
def test_ring_large_grid_two_stages_nn(K):
    plan = dict(bk=32, stages=2, splits=0)
    _run(129, 8328, K, 5, layout='NN', plan=plan)
    _run(129, 8328, K, 5, layout='NN', plan=plan, out_dtype=F32, epi=('bias', 'res'), seed=1)


def test_ring_large_grid_double_buffer_long_k():
    plan = dict(bk=64, stages=2, splits=0)
    _run(129, 8328, 1088, 5, plan=plan)
    _run(129, 8328, 1088, 5, plan=plan, out_dtype=F32, epi=('bias', 'relu'), seed=1)


@pytest.mark.parametrize('M,N,layout', [(8, 8, 'NN'), (8, 327, 'NN'), (129, 8, 'NT'), (129, 327, 'NT'), (129, 327, 'TN')])
def test_ring_edge_tiles(M, N, layout):
    """Edge tiles in both dimensions (M = 8 runs NN: an NT product of at most 32 rows is the skinny kernel's).  K = 64 is below the small-grid ring's
    K >= 128: BK32x3 for k-contiguous B, BK32x2 otherwise; K = 160: the 4-stage ring."""
    st = 3 if layout in ('NT', 'TT') else 2
    for out_dtype, epi in ((BF16, ()), (F32, ('bias', 'res')), (BF16, ('bias', 'relu', 'res'))):
        _run(M, N, 64, 5, layout=layout, plan=dict(bk=32, stages=st), out_dtype=out_dtype, epi=epi)
        _run(M, N, 160, 5, layout=layout, plan=dict(bk=32, stages=4), out_dtype=out_dtype, epi=epi, seed=1)


@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN', 'TT'])
def test_ring_padded_row_strides_and_a_strided_output_view(layout):
    _run(200, 136, 160, 5, layout=layout, plan=dict(bk=32, stages=4), pad=8, out_pad=8, epi=('bias', 'aux', 'res'))
    _run(200, 136, 576, 5, layout=layout, plan=dict(bk=64, stages=4), pad=24, out_pad=16, out_dtype=F32, epi=('bias', 'mul', 'drop', 'res'), seed=1)


def test_ring_full_epilogue_in_the_documented_order():
    for out_dtype in (BF16, F32):
        _run(300, 264, 128, 5, plan=dict(bk=32, stages=4), out_dtype=out_dtype, epi=('bias', 'aux', 'relu', 'mul', 'drop', 'res'), shift=False)


# ------------------------------------------------------------------------------------------- 6: the register-staged kernel
@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN', 'TT'])
@pytest.mark.parametrize('M,N,K', [(70, 50, 37), (200, 136, 264)])
def test_register_staged_k_not_a_multiple_of_32(layout, M, N, K):
    plan = dict(bk=64, stages=0, splits=0)
    _run(M, N, K, 6, layout=layout, plan=plan)
    _run(M, N, K, 6, layout=layout, plan=plan, out_dtype=F32, epi=('bias', 'relu', 'res'), seed=1)


@pytest.mark.parametrize('M,N,layout', [(5, 50, 'TT'), (5, 50, 'TN'), (70, 6, 'NT'), (70, 6, 'NN'), (3, 4, 'TN')])
def test_register_staged_fewer_than_8_rows_or_columns(M, N, layout):
    plan = dict(bk=64, stages=0, splits=0)
    _run(M, N, 64, 6, layout=layout, plan=plan)
    _run(M, N, 64, 6, layout=layout, plan=plan, out_dtype=F32, epi=('bias', 'res'), seed=1)


def _safe_tr_cases():
    for layout in LAYOUTS:
        _run(200, 136, 264, 6, layout=layout, plan=dict(bk=64, stages=0))
        _run(200, 136, 160, 6, layout=layout, plan=dict(bk=64, stages=0), out_dtype=F32, epi=('bias', 'res'), seed=1)   # (a ring shape: the switch takes it off the ring)


def test_register_staged_safe_transpose_reads():
    """EMO_GEMM_SAFE_TR=1 (scalar LDS reads instead of the transposing read) is latched at the library's first GEMM: one child process."""
    env = dict(os.environ, EMO_GEMM_SAFE_TR='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'safe_tr'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'safe_tr ok' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize('splits', [2, 4, 8, 3, 5])
def test_splitk_plain_wgrad_workspace_and_atomics(splits):
    """dW[136, 264] over K = 1024 tokens, forced split counts (3: 352 + 352 + 320, 5: 4 x 224 + 128 — ragged last splits): through the workspace
    (+ 16) and through fp32 atomics, each equal to the oracle and therefore to each other, bit for bit; accumulate onto an integer base."""
    env = {'EMO_GEMM_SPLITS': str(splits)}
    ring = dict(bk=64 if splits == 2 else 32, stages=4, splits=splits)
    o_ws, _, _ = _run(136, 264, 1024, 5, layout='TN', out_dtype=F32, flags=16, plan=ring, env=env)
    o_at, _, _ = _run(136, 264, 1024, 5, layout='TN', out_dtype=F32, flags=0, plan=ring, env=dict(env, EMO_GEMM_SPLIT_ATOMIC='1'))
    assert torch.equal(o_ws, o_at)
    _run(136, 264, 1024, 5, layout='TN', out_dtype=F32, flags=16, plan=ring, env=env, accumulate=True, seed=1)
    _run(136, 264, 1024, 5, layout='TN', out_dtype=F32, flags=0, plan=ring, env=dict(env, EMO_GEMM_SPLIT_ATOMIC='1'), accumulate=True, seed=1)


def test_splitk_plain_wgrad_register_staged_long_k():
    """K > 4096 keeps the wgrad layout on the register-staged kernel (the ring takes A stored [K, M] only up to K = 4096)."""
    _run(136, 264, 8192, 6, layout='TN', out_dtype=F32, flags=16, plan=dict(bk=64, stages=0, splits=4), env={'EMO_GEMM_SPLITS': '4'})
    _run(136, 264, 8192, 6, layout='TN', out_dtype=F32, flags=16, plan=dict(bk=64, stages=0, splits=3), env={'EMO_GEMM_SPLITS': '3'}, rowsum='a', seed=1)


@pytest.mark.parametrize('layout', ['NT', 'NN'])
def test_splitk_reduce_and_epilogue_pass(layout):
    """bf16 outputs on a small grid with K >= 1024: 4 splits through the workspace, summed and finished by the reduce-and-epilogue pass (+ 32)."""
    _run(128, 128, 1024, 5, layout=layout, flags=32, plan=dict(bk=32, stages=4, splits=4))                      # its smallest admitted shape
    _run(128, 128, 1024, 5, layout=layout, flags=32, plan=dict(bk=32, stages=4, splits=4), epi=('bias', 'aux', 'relu', 'mul', 'drop', 'res'), seed=1)
    _run(2048, 512, 2048, 5, layout=layout, flags=32, plan=dict(bk=64, stages=4, splits=4), epi=('bias', 'aux', 'relu', 'mul', 'drop', 'res'), seed=2)
    _run(2048, 512, 2048, 5, layout=layout, flags=32, plan=dict(bk=64, stages=4, splits=4), seed=3)
    # switched off: the same product unsplit
    _run(2048, 512, 2048, 5, layout=layout, flags=0, plan=dict(bk=64, stages=4, splits=0), env={'EMO_GEMM_EPI_SPLIT': '0'}, epi=('bias', 'res'), seed=4)


# ------------------------------------------------------------------------------------------- 1: skinny
@pytest.mark.parametrize('K,waves,chunk', [(32, 4, 128), (96, 4, 128), (160, 4, 128), (512, 4, 128), (1024, 8, 128), (1056, 8, 128), (2048, 16, 64), (2080, 16, 64)])
def test_skinny_wave_counts_empty_slices_and_partial_chunks(K, waves, chunk):
    """K = 32 on 4 waves: waves 1 - 3 have an empty K slice; K = 96 / 160 / 1056 / 2080: slices that are no multiple of the chunk; 1024 <= K < 2048:
    the 8-wave instance."""
    plan = dict(bk=chunk, stages=waves, splits=0)
    for M in (1, 17, 32):
        for N in (8, 24, 327):
            _run(M, N, K, 1, plan=plan, epi=('bias', 'relu', 'res'))
            _run(M, N, K, 1, plan=plan, out_dtype=F32, epi=('bias', 'relu', 'res'), seed=1)
    _run(17, 327, K, 1, plan=plan, seed=2)
    _run(32, 24, K, 1, plan=plan, out_dtype=F32, epi=('bias', 'aux', 'relu', 'mul', 'drop', 'res'), seed=3)       # (the slow epilogue of wave 0)


# ------------------------------------------------------------------------------------------- 2: A-stationary K = 512
def _min_rows():
    return _ops().ASTAT_MIN_ROWS


COL_SPLIT = {64: 1, 128: 1, 512: 4, 2048: 16}      # 32 / 33 row panels: the smallest split that fills the chip, at most N / 128 (emo_gemm_astat.hip)


@pytest.mark.parametrize('extra_rows', [0, 128])
@pytest.mark.parametrize('N', [64, 128, 512, 2048])
def test_astat_column_split_from_the_plan(extra_rows, N):
    M = _min_rows() + extra_rows
    plan = dict(bk=128, stages=4, splits=0, col=COL_SPLIT[N])
    _run(M, N, 512, 2, plan=plan)                                                        # plain
    _run(M, N, 512, 2, plan=plan, epi=('bias', 'relu'), seed=1)                          # ReLU
    _run(M, N, 512, 2, plan=plan, out_dtype=F32, epi=('bias', 'res'), seed=2)            # generic: fp32 out


@pytest.mark.parametrize('extra_rows', [0, 128])
def test_astat_one_case_per_exact_instantiation(extra_rows):
    M, N = _min_rows() + extra_rows, 512
    plan = dict(bk=128, stages=4, col=4)
    _run(M, N, 512, 2, plan=plan, epi=('res',))                                          # residual
    _run(M, N, 512, 2, plan=plan, epi=('bias', 'drop', 'res'), seed=1)                   # dropout + residual
    _run(M, N, 512, 2, plan=plan, epi=('mul',), seed=2)                                  # generic: NONZERO
    _run(M, N, 512, 2, plan=plan, epi=('bias', 'aux', 'relu', 'mul', 'drop', 'res'), seed=3, shift=False)
    _, exp, mask = _run(M, N, 512, 2, plan=plan, epi=('bias', 'relu', 'drop'), mask_out=True, seed=4)       # ReLU + dropout + mask_out
    assert 0.1 < float(exp.mask.mean()) < 0.4
    _run(M, N, 512, 2, plan=plan, bitmask=(mask, exp.mask), seed=5)                      # BITMASK multiply fed by that mask
    _run(M, N, 512, 2, plan=dict(plan, col=2), env={'EMO_ASTAT_SPLIT': '2'}, epi=('bias', 'relu'), seed=6)   # a forced column split


def test_astat_mask_across_sixteen_column_blocks():
    M, N = _min_rows(), 2048
    plan = dict(bk=128, stages=4, col=16)
    _, exp, mask = _run(M, N, 512, 2, plan=plan, epi=('bias', 'relu', 'drop'), mask_out=True)
    _run(M, N, 512, 2, plan=plan, bitmask=(mask, exp.mask), seed=1)


def test_astat_strided_views_and_refusals():
    ops = _ops()
    from emo_disentanger_amd._lib import EmoError
    M, N, K = _min_rows(), 512, 512
    _run(M, N, K, 2, plan=dict(bk=128, stages=4, col=4), pad=512, out_pad=8, epi=('bias', 'res'))
    # an output row stride that is no multiple of 8 elements: refused, the ring takes it (one block per tile, unsplit: a strided C) and stays exact
    _run(M, N, K, 5, plan=dict(bk=64, stages=4, splits=0), out_pad=4, epi=('bias', 'res'), seed=1)
    _run(M + 64, N, K, (5, 6), out_pad=0, epi=('bias', 'relu'), seed=2)                  # M % 128 != 0
    # an A operand one element off its 16-byte alignment: no bf16 kernel takes it, and none may be run on it silently
    flat = X.ints((M * K + 8,), -3, 3, 1).cuda()
    A1, W = flat[1:1 + M * K].view(M, K), X.ints((N, K), -3, 3, 2).cuda()
    assert A1.data_ptr() % 16 == 2
    with pytest.raises(EmoError, match='aligned'):
        ops.gemm(A1, W)
    with pytest.raises(EmoError, match='mask_out'):
        ops.gemm(A1, W, act=ops.ACT_RELU, mask_out=torch.zeros(M, N // 8, device='cuda', dtype=torch.uint8))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 4: 256 x 256 NT
@pytest.mark.parametrize('M,N,K', [(256, 256, 256), (512, 256, 320), (256, 512, 1088)])
def test_256_tile_nt(M, N, K):
    env, plan = {'EMO_GEMM_W128': '1'}, dict(bk=64, stages=3, splits=0)
    for i, epi in enumerate(((), ('bias',), ('res',), ('bias', 'drop', 'res'))):
        _run(M, N, K, 4, plan=plan, env=env, epi=epi, seed=i)
    _run(M, N, K, 5, env={'EMO_GEMM_W128': '0'}, epi=('bias', 'res'), seed=9)            # the other side of the switch


# ------------------------------------------------------------------------------------------- 3: 256 x 256 wgrad
def test_256_tile_wgrad_default_thresholds():
    ops = _ops()
    _run(1024, 768, 8192, 3, layout='TN', out_dtype=F32, plan=dict(bk=64, stages=3, splits=8))
    assert ops.lib.emo_gemm_workspace_bytes(1024, 768, 8192, 1, 0) >= 8 * 1024 * 768 * 4


LOW = {'EMO_W128_TN_MINKT': '1', 'EMO_W128_TN_MINBLK': '1'}


@pytest.mark.parametrize('M,N,K,splits', [(256, 256, 4096, 64), (256, 512, 4096, 64), (768, 256, 4096, 64), (256, 1280, 4096, 51), (512, 768, 4096, 42),
                                          (768, 1024, 2048, 21), (768, 1024, 8192, 21)])
def test_256_tile_wgrad_lowered_thresholds(M, N, K, splits):
    """1, 2, 3, 5, 6 and 12 tiles: 8 f + x splits with f whole splits per XCD and x `extra` ones in the slots left over (5 tiles: 6 + 3, 6: 5 + 2,
    12: 2 + 5); the workspace size follows the same plan."""
    ops = _ops()
    plan = dict(bk=64, stages=3, splits=splits)
    _run(M, N, K, 3, layout='TN', out_dtype=F32, plan=plan, env=LOW)
    with _Env(LOW):
        need = ops.lib.emo_gemm_workspace_bytes(M, N, K, 1, 0)
    assert need >= splits * M * N * 4
    _run(M, N, K, 3, layout='TN', out_dtype=F32, plan=plan, env=LOW, accumulate=True, rowsum='a', seed=1)


def test_256_tile_wgrad_bias_gradients_and_small_workspaces():
    M, N, K, splits = 512, 768, 4096, 42
    plan = dict(bk=64, stages=3, splits=splits)
    _run(M, N, K, 3, layout='TN', out_dtype=F32, plan=plan, env=LOW, rowsum='a')                      # nn.Linear layout: dY is the A operand
    _run(M, N, K, 3, layout='TN', out_dtype=F32, plan=plan, env=LOW, rowsum='b', seed=1)              # Conv1D layout: dY is the B operand
    # room for the product's partials only: the bias gradient leaves the kernel through atomics
    _run(M, N, K, 3, layout='TN', out_dtype=F32, plan=plan, env=LOW, rowsum='a', ws_bytes=lambda need: splits * M * N * 4, seed=2)
    _run(M, N, K, 3, layout='TN', out_dtype=F32, plan=plan, env=LOW, rowsum='b', ws_bytes=lambda need: splits * M * N * 4, accumulate=True, seed=3)
    # too small for the product: the 128 x 128 kernels take it, split as far as the workspace goes
    _run(M, N, K, (5, 6), layout='TN', out_dtype=F32, flags=16, env=LOW, ws_bytes=lambda need: splits * M * N * 4 - 16, seed=4)
    _run(M, N, K, (5, 6), layout='TN', out_dtype=F32, flags=0, env=LOW, ws_bytes=lambda need: 0, rowsum='a', seed=5)       # none at all: atomics


# ------------------------------------------------------------------------------------------- 7: fp32
@pytest.mark.parametrize('layout', ['NT', 'NN', 'TN', 'TT'])
@pytest.mark.parametrize('M,N,K', [(128, 128, 16), (129, 327, 509), (70, 50, 37)])
def test_fp32_tiles_and_unaligned_strides(layout, M, N, K):
    for pad in (0, 3):                                               # 3: row strides that are no multiple of 4 elements (vector loads off)
        for env in (None, {'EMO_GEMM_F32_TILE': '64'}):              # the 128-tile plan where M, N >= 128, and the 64-tile kernel on the same shape
            _run(M, N, K, 7, layout=layout, in_dtype=F32, out_dtype=F32, plan=dict(bk=16, stages=0, splits=0), pad=pad, env=env,
                 epi=('bias', 'relu', 'res'), seed=pad)
    _run(M, N, K, 7, layout=layout, in_dtype=F32, out_dtype=F32, plan=dict(bk=16, stages=0), epi=('bias', 'aux', 'relu', 'mul', 'drop', 'res'), seed=5)


@pytest.mark.parametrize('M,N', [(136, 72), (136, 264)])
def test_fp32_split_k(M, N):
    """The 64-tile (N < 128) and the 128-tile plan, forced to 5 splits of a K = 4224 reduction (4 x 848 + 832)."""
    for env in ({'EMO_GEMM_SPLITS': '5'}, {'EMO_GEMM_SPLITS': '5', 'EMO_GEMM_SPLIT_ATOMIC': '1'}):
        flags = 0 if 'EMO_GEMM_SPLIT_ATOMIC' in env else 16
        _run(M, N, 4224, 7, layout='TN', in_dtype=F32, out_dtype=F32, flags=flags, plan=dict(bk=16, splits=5), env=env)
        _run(M, N, 4224, 7, layout='TN', in_dtype=F32, out_dtype=F32, flags=flags, plan=dict(bk=16, splits=5), env=env, accumulate=True, rowsum='a', seed=1)


if __name__ == '__main__':
    if sys.argv[1:] == ['safe_tr']:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        _safe_tr_cases()
        print('safe_tr ok')
