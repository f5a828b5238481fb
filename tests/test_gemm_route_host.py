"""emo_gemm's planner on the host: emo_gemm_route launches nothing and needs no GPU, so the route table that tests/test_gpu_gemm_exact.py asserts on the
device (family, split flags, plan fields — see its docstring for the families and their edge shapes) is asserted here on every machine, with the
refusals, the purity of the query, and emo_gemm_workspace_bytes against the sizes the library returned before it had a planner
(tests/golden/gemm_workspace_bytes.json, written by tools/gemm_workspace_golden.py).  Operand pointers are small fake addresses, 16-byte aligned."""
import ctypes
import json
import os

import pytest
import torch

from emo_disentanger_amd import _lib, ops
from emo_disentanger_amd._lib import BF16, F32, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {'NT': (0, 0), 'NN': (0, 1), 'TT': (1, 0), 'TN': (1, 1)}    # (a_trans, b_trans): A stored [K, M] / B stored [K, N]
PA, PB, PC, PW, PX = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
LOW = {'EMO_W128_TN_MINKT': '1', 'EMO_W128_TN_MINBLK': '1'}
GOLDEN = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'gemm_workspace_bytes.json')))


class _Env:
    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def _args(M, N, K, layout, din, dout, ws, accumulate=False, A=PA, out_pad=0, **epi):
    """Arguments of emo_gemm / emo_gemm_route (without the trailing stream / result pointers) for contiguous operands whose bf16 rows are padded to
    16 bytes; ws: workspace bytes offered (None: what emo_gemm_workspace_bytes asks for); epi: Epilogue fields (pointer fields: any true value)."""
    a_t, b_t = LAYOUTS[layout]
    pad = (lambda n: (n + 7) // 8 * 8) if din == BF16 else (lambda n: n)
    if ws is None:
        ws = lib.emo_gemm_workspace_bytes(M, N, K, din, dout)
    e = _lib.Epilogue()
    e.mul_scale = 1.0
    for k, v in epi.items():
        setattr(e, k, v if k in ('act', 'mul_mode', 'p_drop', 'hdiv_T', 'mul_scale') else PX)
    if ws:
        e.workspace, e.workspace_bytes = PW, ws
    return [A, a_t, pad(M if a_t else K), PB, b_t, pad(N if b_t else K), PC, N + out_pad, M, N, K, din, dout, int(accumulate), ctypes.byref(e)], e


def route(M, N, K, layout='NT', din=BF16, dout=BF16, ws=None, env=None, **kw):
    """(family, flags, plan fields) of emo_gemm_route, or the error text."""
    with _Env(env):
        args, keep = _args(M, N, K, layout, din, dout, ws, **kw)
        code, plan = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.emo_gemm_route(*args, ctypes.byref(code), ctypes.byref(plan))
    if rc:
        return lib.emo_last_error().decode()
    c, p = code.value, plan.value
    return c & 15, c & 48, dict(bk=p & 255, stages=(p >> 8) & 255, splits=(p >> 16) & 255, col=(p >> 24) & 255)


def expect(fam, flags, plan, *a, **kw):
    got = route(*a, **kw)
    assert not isinstance(got, str), (got, a, kw)
    assert got[0] == fam and got[1] == flags, (got, a, kw)
    for k, v in plan.items():
        assert got[2][k] == v, (k, got, a, kw)


EPI = dict(bias=1, residual=1)


# ------------------------------------------------------------------------------------------- the route table
@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_ring_routes(layout):
    for K, bk in ((128, 32), (160, 32), (512, 64), (576, 64)):                            # small grid: the 4-stage ring
        expect(5, 0, dict(bk=bk, stages=4, splits=0), 200, 136, K, layout)
        expect(5, 0, dict(bk=bk, stages=4, splits=0), 200, 136, K, layout, dout=F32, **EPI)
    st = 3 if layout in ('NT', 'TT') else 2                                               # large grid: 3 stages for k-contiguous B, else 2
    for K in (32, 64, 96, 128):
        expect(5, 0, dict(bk=32, stages=st, splits=0), 129, 8328, K, layout)
        expect(5, 0, dict(bk=32, stages=st, splits=0), 129, 8328, K, layout, dout=F32, **EPI)
    expect(5, 0, dict(bk=64, stages=2, splits=0) if st == 3 else dict(bk=32, stages=2, splits=0), 129, 8328, 1088, layout)
    expect(5, 0, dict(bk=32, stages=st, splits=0), 8328, 1024, 64, layout, dout=F32, bias=1)
    for M, N in ((8, 8), (8, 327), (129, 8), (129, 327)):                                 # edge tiles; K = 64 is below the small-grid ring's K >= 128
        if layout == 'NT' and M <= 32:
            continue                                                                      # (the skinny kernel's)
        expect(5, 0, dict(bk=32, stages=st), M, N, 64, layout)
        expect(5, 0, dict(bk=32, stages=4), M, N, 160, layout, dout=F32, **EPI)
    expect(5, 0, dict(bk=32, stages=4), 200, 136, 160, layout, out_pad=8, aux_out=1, **EPI)       # a strided output view


@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_register_staged_routes(layout):
    plan = dict(bk=64, stages=0, splits=0)
    for M, N, K in ((70, 50, 37), (200, 136, 264)):
        expect(6, 0, plan, M, N, K, layout)
        expect(6, 0, plan, M, N, K, layout, dout=F32, act=ops.ACT_RELU, **EPI)
    for M, N in ((5, 50), (70, 6), (3, 4)):
        if layout == 'NT' and M <= 32:
            continue
        expect(6, 0, plan, M, N, 64, layout)


def test_split_k_routes():
    for s in (2, 4, 8, 3, 5):
        ring = dict(bk=64 if s == 2 else 32, stages=4, splits=s)
        expect(5, 16, ring, 136, 264, 1024, 'TN', dout=F32, env={'EMO_GEMM_SPLITS': str(s)})
        expect(5, 0, ring, 136, 264, 1024, 'TN', dout=F32, env={'EMO_GEMM_SPLITS': str(s), 'EMO_GEMM_SPLIT_ATOMIC': '1'})
        expect(5, 16, ring, 136, 264, 1024, 'TN', dout=F32, env={'EMO_GEMM_SPLITS': str(s)}, accumulate=True)
    # K > 4096 keeps the wgrad layout on the register-staged kernel, the bias gradient in-kernel
    expect(6, 16, dict(bk=64, stages=0, splits=4), 136, 264, 8192, 'TN', dout=F32, env={'EMO_GEMM_SPLITS': '4'})
    expect(6, 16, dict(bk=64, stages=0, splits=3), 136, 264, 8192, 'TN', dout=F32, env={'EMO_GEMM_SPLITS': '3'}, a_rowsum=1)
    for layout in ('NT', 'NN'):                                                           # the reduce-and-epilogue pass
        full = dict(bias=1, aux_out=1, act=ops.ACT_RELU, mul_aux=1, mul_mode=ops.MUL_NONZERO, p_drop=0.5, residual=1)
        expect(5, 32, dict(bk=32, stages=4, splits=4), 128, 128, 1024, layout)
        expect(5, 32, dict(bk=32, stages=4, splits=4), 128, 128, 1024, layout, **full)
        expect(5, 32, dict(bk=64, stages=4, splits=4), 2048, 512, 2048, layout, **full)
        expect(5, 32, dict(bk=64, stages=4, splits=4), 2048, 512, 2048, layout)
        expect(5, 0, dict(bk=64, stages=4, splits=0), 2048, 512, 2048, layout, env={'EMO_GEMM_EPI_SPLIT': '0'}, **EPI)


def test_skinny_routes():
    for K, waves, chunk in ((32, 4, 128), (96, 4, 128), (160, 4, 128), (512, 4, 128), (1024, 8, 128), (1056, 8, 128), (2048, 16, 64), (2080, 16, 64)):
        for M in (1, 17, 32):
            for N in (8, 24, 327):
                for dout in (BF16, F32):
                    expect(1, 0, dict(bk=chunk, stages=waves, splits=0), M, N, K, dout=dout, act=ops.ACT_RELU, **EPI)


def test_astat_routes():
    rows = ops.ASTAT_MIN_ROWS
    assert rows == 4096
    for M in (rows, rows + 128):
        for N, col in ((64, 1), (128, 1), (512, 4), (2048, 16)):
            plan = dict(bk=128, stages=4, splits=0, col=col)
            expect(2, 0, plan, M, N, 512)
            expect(2, 0, plan, M, N, 512, bias=1, act=ops.ACT_RELU)
            expect(2, 0, plan, M, N, 512, dout=F32, **EPI)
        expect(2, 0, dict(col=4), M, 512, 512, bias=1, act=ops.ACT_RELU, p_drop=0.5, mask_out=1)
        expect(2, 0, dict(col=4), M, 512, 512, mul_aux=1, mul_mode=ops.MUL_BITMASK)
        expect(2, 0, dict(col=2), M, 512, 512, env={'EMO_ASTAT_SPLIT': '2'})
    expect(5, 0, dict(bk=64, stages=4, splits=0), rows, 512, 512, out_pad=4, **EPI)       # an output row stride that is no multiple of 8: the ring
    assert route(rows + 64, 512, 512, bias=1)[0] in (5, 6)
    assert route(rows, 512, 512, env={'EMO_GEMM_NO_ASTAT': '1'})[0] == 5
    assert route(rows, 512, 512, env={'EMO_ASTAT_MIN_ROWS': '8192'})[0] == 5 and route(2048, 512, 512, env={'EMO_ASTAT_MIN_ROWS': '2048'})[0] == 2


def test_256_tile_routes():
    for M, N, K in ((256, 256, 256), (512, 256, 320), (256, 512, 1088)):
        for epi in ({}, dict(bias=1), dict(residual=1), dict(bias=1, p_drop=0.5, residual=1)):
            expect(4, 0, dict(bk=64, stages=3, splits=0), M, N, K, env={'EMO_GEMM_W128': '1'}, **epi)
        assert route(M, N, K, env={'EMO_GEMM_W128': '0'}, **EPI)[0] == 5
    expect(4, 0, dict(bk=64, stages=3), 131072, 512, 2048, bias=1, residual=1, p_drop=0.1)      # default thresholds: the long-K forward products of a step
    expect(3, 0, dict(bk=64, stages=3, splits=8), 1024, 768, 8192, 'TN', dout=F32)
    for M, N, K, s in ((256, 256, 4096, 64), (256, 512, 4096, 64), (768, 256, 4096, 64), (256, 1280, 4096, 51), (512, 768, 4096, 42), (768, 1024, 2048, 21),
                       (768, 1024, 8192, 21)):
        expect(3, 0, dict(bk=64, stages=3, splits=s), M, N, K, 'TN', dout=F32, env=LOW)
        expect(3, 0, dict(bk=64, stages=3, splits=s), M, N, K, 'TN', dout=F32, env=LOW, accumulate=True, a_rowsum=1)
    M, N, K, s = 512, 768, 4096, 42
    expect(3, 0, dict(splits=s), M, N, K, 'TN', dout=F32, env=LOW, b_rowsum=1, ws=s * M * N * 4)             # no room for the bias partials: still this kernel
    got = route(M, N, K, 'TN', dout=F32, env=LOW, ws=s * M * N * 4 - 16)                                     # too small for the product
    assert got[0] in (5, 6) and got[1] == 16
    got = route(M, N, K, 'TN', dout=F32, env=LOW, ws=0, a_rowsum=1)
    assert got[0] in (5, 6) and got[1] == 0


@pytest.mark.parametrize('layout', list(LAYOUTS))
def test_fp32_routes(layout):
    for M, N, K in ((128, 128, 16), (129, 327, 509), (70, 50, 37)):
        for env in (None, {'EMO_GEMM_F32_TILE': '64'}):
            expect(7, 0, dict(bk=16, stages=0, splits=0), M, N, K, layout, F32, F32, env=env, act=ops.ACT_RELU, **EPI)
    for M, N in ((136, 72), (136, 264)):
        expect(7, 16, dict(bk=16, splits=5), M, N, 4224, layout, F32, F32, env={'EMO_GEMM_SPLITS': '5'})
        expect(7, 0, dict(bk=16, splits=5), M, N, 4224, layout, F32, F32, env={'EMO_GEMM_SPLITS': '5', 'EMO_GEMM_SPLIT_ATOMIC': '1'})


# ------------------------------------------------------------------------------------------- refusals, purity
LNA = dict(lna_gamma=1, lna_beta=1, lna_out=1, lna_mean=1, lna_rstd=1)


@pytest.mark.parametrize('what,a,kw', [
    ('lna_* (LayerNorm of the A operand) exists only on the A-stationary kernel', (4096, 512, 256), LNA),                     # outside the class by shape
    ('lna_* (LayerNorm of the A operand) exists only on the A-stationary kernel: bf16, NT', (4096, 512, 512), dict(LNA, env={'EMO_GEMM_NO_ASTAT': '1'})),
    ('hdiv exists only on the A-stationary kernel (K = 512', (4096, 512, 1024), dict(hdiv=1, hdiv_T=2048)),
    ('hdiv exists only on the A-stationary kernel and this call was refused by it', (4096, 512, 512), dict(hdiv=1, hdiv_T=2048, env={'EMO_GEMM_NO_ASTAT': '1'})),
    ('mask_out / EMO_MUL_BITMASK need bf16 in/out, NT, K = 512', (200, 512, 512), dict(mask_out=1, act=ops.ACT_RELU)),
    ('mask_out / EMO_MUL_BITMASK need bf16 in/out, NT, K = 512', (4096, 512, 512), dict(mul_aux=1, mul_mode=ops.MUL_BITMASK, A=PA + 2)),
    ('emo_gemm(bf16): A/B must be 16-B aligned', (4096, 512, 512), dict(A=PA + 2)),
    ('emo_gemm: accumulate needs fp32 output', (200, 136, 128), dict(accumulate=True)),
])
def test_route_and_gemm_refuse_with_the_same_message(what, a, kw):
    """(emo_gemm with no stream: every one of these is refused before anything is launched)"""
    kw = dict(kw)
    env = kw.pop('env', None)
    got = route(*a, env=env, **kw)
    assert isinstance(got, str) and what in got, got
    with _Env(env):
        args, keep = _args(*a, 'NT', BF16, BF16, None, **kw)
        assert lib.emo_gemm(*args, None) == -1
        assert lib.emo_last_error().decode() == got


def test_route_leaves_the_last_kernel_and_plan_words_alone():
    before = lib.emo_gemm_last_kernel(), lib.emo_gemm_last_plan()
    for a in ((200, 136, 128), (4096, 512, 512), (17, 327, 512), (128, 128, 1024)):
        assert not isinstance(route(*a), str)
    assert isinstance(route(200, 512, 512, mask_out=1), str)
    assert (lib.emo_gemm_last_kernel(), lib.emo_gemm_last_plan()) == before


# ------------------------------------------------------------------------------------------- workspace sizes
def test_workspace_bytes_are_what_they_were_before_the_planner():
    assert len(GOLDEN['rows']) > 1000
    for M, N, K, din, dout, e, want in GOLDEN['rows']:
        with _Env(GOLDEN['envs'][e]):
            assert lib.emo_gemm_workspace_bytes(M, N, K, din, dout) == want, (M, N, K, din, dout, GOLDEN['envs'][e])


def test_a_workspace_of_the_size_asked_for_is_always_used():
    """Every layout of every golden shape, offered exactly emo_gemm_workspace_bytes: a split product goes through the workspace (+ 16 / + 32), never
    through atomics.  The 256 x 256 wgrad kernel (family 3) has no other way out than the workspace and reports no flag.
    Exception, as before the planner: M * N % 4 != 0 — the reduce pass works on 16-byte pieces, the size query does not look at that."""
    n = 0
    for M, N, K, din, dout, e, want in GOLDEN['rows']:
        if din == F32 and dout == BF16:
            continue
        for layout in LAYOUTS:
            got = route(M, N, K, layout, din, dout, env=GOLDEN['envs'][e])
            if isinstance(got, str):
                continue
            fam, flags, plan = got
            if plan['splits'] > 1 and fam != 3 and (M * N) % 4 == 0:
                assert flags in (16, 32), (M, N, K, layout, din, dout, got, want)
                n += 1
            if fam == 3:
                assert want >= plan['splits'] * M * N * 4
    assert n > 100


# ------------------------------------------------------------------------------------------- the Python side asks the library
def test_ops_predicates_are_the_library_query():
    for env in (None, {'EMO_GEMM_NO_ASTAT': '1'}, {'EMO_ASTAT_MIN_ROWS': '8192'}, {'EMO_ASTAT_MIN_ROWS': '1024'}):
        with _Env(env):
            assert ops.ASTAT_MIN_ROWS == lib.emo_gemm_astat_min_rows() == (int(env['EMO_ASTAT_MIN_ROWS']) if env and 'EMO_ASTAT_MIN_ROWS' in env else 4096)
            for M in (1024, 4096, 4160, 8192):
                for N in (32, 64, 512, 2048, 2112):
                    for K in (512, 1024):
                        want = bool(lib.emo_gemm_astat_supported(BF16, BF16, M, N, K))
                        assert want == (K == 512 and M % 128 == 0 and M >= ops.ASTAT_MIN_ROWS and N % 64 == 0 and 64 <= N <= 2048 and not (env and 'EMO_GEMM_NO_ASTAT' in env))
                        assert ops.gemm_lna_ok(M, N, K, torch.bfloat16) == want and ops.gemm_bitmask_ok(M, N, K, torch.bfloat16, torch.bfloat16) == want
                        assert not ops.gemm_lna_ok(M, N, K, torch.float32) and not ops.gemm_bitmask_ok(M, N, K, torch.bfloat16, torch.float32)
                        assert (route(M, N, K)[0] == 2) == want
    with _Env({'EMO_LN_IN_GEMM': '0'}):
        assert not ops.gemm_lna_ok(4096, 512, 512, torch.bfloat16) and ops.gemm_bitmask_ok(4096, 512, 512, torch.bfloat16, torch.bfloat16)
