"""Thin tensor-level wrappers over the C-ABI (no autograd here; see model/ for the autograd glue).

Every function takes GPU tensors, validates layout, and launches on torch's current stream.
2-D operands may be row-strided views (``stride(1) == 1``), e.g. the q/k/v slices of a fused
projection."""
import ctypes

import os

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_GELU_NEW, ACT_NONE, ACT_RELU, ATTN_BWD, ATTN_BWD_KV, ATTN_BWD_R, ATTN_DECODE, ATTN_FAVOR, ATTN_FWD, ATTN_RELPOS, ATTN_SOFTMAX, BF16, F32, MUL_BITMASK, MUL_DGELU, MUL_DGELU_NEW, MUL_NONE, MUL_NONZERO, GRAMMAR_ACC, GRAMMAR_ACC_QUEUE, GRAMMAR_ACC_WINDOW, GRAMMAR_TXL, GRAMMAR_TXL_QUEUE, Attn, DecodeStep, Epilogue, GrammarStep, check,
                   dtype_code, lib, ptr, stream)

__all__ = ['gemm', 'colsum', 'embed_fwd', 'embed_bwd', 'layernorm_fwd', 'layernorm_bwd', 'dropout_apply', 'favor_attn_fwd',
           'favor_attn_bwd', 'favor_decode_step', 'decode_step', 'decode_step_set', 'block_set', 'DecodeStep', 'GrammarStep', 'grammar_step', 'draw_score_tables', 'guide_pairs_error', 'favor_draw_omega', 'favor_state_reset', 'favor_state_at', 'acc_rebase', 'softmax_attn_fwd', 'softmax_attn_bwd', 'softmax_attn_decode', 'relpos_attn_fwd', 'relpos_attn_bwd', 'relpos_attn_decode', 'xent_fwd',
           'xent_bwd', 'token_scores', 'xent_bwd_rows', 'argmax', 'sample_nucleus', 'sample_nucleus_step', 'txl_grammar_step', 'txl_queue_step', 'acc_grammar_step', 'acc_queue_step', 'acc_window_step', 'accuracy_counts', 'sumsq', 'clip_coef', 'adam_step', 'cast', 'add_bias2',
           'ACT_NONE', 'ACT_RELU', 'ACT_GELU_NEW', 'ACT_GELU', 'MUL_NONE', 'MUL_NONZERO', 'MUL_DGELU_NEW', 'MUL_DGELU', 'MUL_BITMASK', 'gemm_astat_ok', 'gemm_bitmask_ok', 'gemm_lna_ok', 'bitmask_rows', 'favor_bwd_dn_ok', 'ffn_fwd', 'ffn_fwd_ok']


def _c(t):
    """contiguous int64 tensor (or None).  NEVER call .contiguous() inside a ptr(...) argument: the temporary dies before
    the launch and the caching allocator hands its block to the next temporary."""
    if t is None:
        return None
    assert t.dtype == torch.int64
    return t if t.is_contiguous() else t.contiguous()


def _rows(t):
    assert t.dim() == 2 and t.stride(1) == 1, 'need a 2-D tensor with unit column stride'
    return t.stride(0)


_stream = stream   # (gemm() has a keyword argument of that name)
_ws_cache = {}
_ws_need = {}      # emo_gemm_workspace_bytes by problem (a pure function of the shape: one library call per shape, not per launch)
GEMM_TIMING = None   # bench.py sets this to a list: every GEMM launch is then bracketed by HIP events on its launch stream (in situ)
KERNEL_TIMING = None  # bench.py sets this to a dict kind -> list of (event0, event1, algorithmic flops, algorithmic bytes) for the attention kernels


class _timed:
    """with _timed(kind, flops, bytes): brackets the launches inside with HIP events on torch's current stream when bench.py asked for it."""

    def __init__(self, kind, flops, nbytes):
        self.kind, self.flops, self.nbytes = kind, flops, nbytes

    def __enter__(self):
        if KERNEL_TIMING is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *a):
        if KERNEL_TIMING is not None:
            self.e1.record()
            KERNEL_TIMING.setdefault(self.kind, []).append((self.e0, self.e1, self.flops, self.nbytes))
        return False


def _workspace(kind, device, need, st=None):
    """Caller-owned kernel scratch (the library never allocates): one buffer per (kind, device, stream), grown on demand.  Consumers on one
    stream run in launch order, so consecutive launches can share it.  The size REPORTED to the kernel is the size it asked for, not the
    (possibly larger) cached buffer: the GEMM's split-K count depends on the workspace it is offered, and a result must not depend on which
    shapes the process happened to run before (r03: a trace test passed alone and failed after other tests by 1e-4 of a parameter sum)."""
    if need == 0:
        return None, 0
    key = (kind, device, st if st is not None else stream())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < need:
        if buf is not None and st is not None and st != stream():
            # (r05 advisor finding) the scratch of a side-stream launch is allocated from the CURRENT stream's pool: the buffer that is being
            # replaced may still be in use by an earlier launch on `st`, and without this mark the caching allocator would hand its block to the
            # next main-stream allocation as soon as the reference drops
            buf.record_stream(torch.cuda.ExternalStream(st))
        buf = torch.empty(need, device=device, dtype=torch.uint8)
        _ws_cache[key] = buf
    return buf, need


def gemm(A, B, *, a_trans=False, b_trans=False, out=None, out_dtype=None, accumulate=False, bias=None, act=ACT_NONE,
         aux_out=None, mul_aux=None, mul_mode=MUL_NONE, mul_scale=1.0, p_drop=0.0, seed=0, offset=0, residual=None,
         ln_c1=None, ln_eps=1e-5, ln_stats_out=None, rln=None, a_rowsum=None, b_rowsum=None, mask_out=None, stream=None, lna=None, lna_out=None, hdiv=None):
    """C[M,N] = epilogue(op(A) @ op(B));  a_trans: A stored [K,M];  b_trans=False: B stored [N,K] (nn.Linear),
    b_trans=True: B stored [K,N] (HF Conv1D).  ln_c1 / ln_stats_out / rln: LayerNorm folded around a decode-step GEMM (include/emo_hip.h).
    stream: raw hipStream_t to launch on (default: torch's current stream).
    lna = (gamma, beta, eps): A is the RAW input of a LayerNorm whose output is the operand — the A-stationary kernel normalises its row panel in
    registers (gemm_lna_ok shapes only); returns (C, LN(A), mean, rstd) instead of C."""
    st = stream if stream is not None else _stream()
    K, M = (A.shape if a_trans else A.shape[::-1])
    Kb, N = (B.shape if b_trans else B.shape[::-1])
    assert K == Kb, 'inner dims differ: %s vs %s' % (tuple(A.shape), tuple(B.shape))
    assert A.dtype == B.dtype
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=out_dtype or A.dtype)
    ws, ws_bytes = None, 0
    plain = bias is None and residual is None and aux_out is None and mul_aux is None and act == ACT_NONE and p_drop == 0.0
    if (out.dtype == torch.float32 and plain) or (out.dtype == torch.bfloat16 and not accumulate and M > 32):
        # fp32 plain outputs (wgrad): split-K partial sums; bf16 outputs on a small tile grid with a long reduction: split-K + reduce-with-epilogue
        wkey = (M, N, K, A.dtype, out.dtype)
        need = _ws_need.get(wkey)
        if need is None:
            need = _ws_need[wkey] = lib.emo_gemm_workspace_bytes(M, N, K, dtype_code(A.dtype), dtype_code(out.dtype))
        ws, ws_bytes = _workspace('gemm', A.device, need, st)
    rx, rstats, rgamma, rbeta = rln if rln is not None else (None, None, None, None)     # residual = LayerNorm(rx) from exported statistics
    assert rx is None or (rx.dtype == out.dtype and _rows(rx) == _rows(out))
    ln_out = ln_mean = ln_rstd = None
    if lna is not None:
        assert gemm_lna_ok(M, N, K, A.dtype) and not a_trans and not b_trans and lna[0].dtype == torch.float32 and lna[1].dtype == torch.float32
        assert _rows(A) % 8 == 0 and _rows(B) % 8 == 0 and _rows(out) % 8 == 0 and (A.data_ptr() | B.data_ptr() | out.data_ptr()) % 16 == 0, \
            'lna=: the A-stationary kernel needs 16-B aligned operands and row strides that are multiples of 8 elements'
        ln_eps = lna[2]
        if lna_out is not None:                                    # caller's (rows, mean, rstd) buffers: row chunks of one tensor
            ln_out, ln_mean, ln_rstd = lna_out
            assert ln_out.shape == (M, K) and ln_out.is_contiguous() and ln_out.dtype == A.dtype and ln_mean.numel() == M and ln_rstd.numel() == M
        else:
            ln_out = torch.empty(M, K, device=A.device, dtype=A.dtype)
            ln_mean = torch.empty(M, device=A.device, dtype=torch.float32)
            ln_rstd = torch.empty(M, device=A.device, dtype=torch.float32)
    epi = Epilogue(ptr(bias), act, ptr(aux_out), ptr(mul_aux), mul_mode, mul_scale, p_drop, seed, offset, ptr(residual),
                   ptr(ln_c1), ln_eps, ptr(ln_stats_out), ptr(rx), ptr(rstats), ptr(rgamma), ptr(rbeta), ptr(a_rowsum), ptr(b_rowsum), ptr(mask_out), ptr(ws), ws_bytes,
                   ptr(lna[0]) if lna is not None else None, ptr(lna[1]) if lna is not None else None, ptr(ln_out), ptr(ln_mean), ptr(ln_rstd),
                   ptr(hdiv[0]) if hdiv is not None else None, int(hdiv[1]) if hdiv is not None else 0)
    if hdiv is not None:      # (den, T): C[m][n] /= den[m / T, n / 64, m % T]  (emo_hip.h: hdiv — the out-projection dgrad leaves dN = dout / den)
        assert hdiv[0].dtype == torch.float32 and hdiv[0].is_contiguous() and hdiv[0].numel() == M * (N // 64) and plain and mask_out is None and lna is None
    if not plain or mask_out is not None:
        for t in (aux_out, residual) + (() if mul_mode == MUL_BITMASK else (mul_aux,)):
            assert t is None or (t.dtype == out.dtype and _rows(t) == _rows(out))
        for t in (mask_out,) + ((mul_aux,) if mul_mode == MUL_BITMASK else ()):
            assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.shape == (M, N // 8) and gemm_bitmask_ok(M, N, K, A.dtype, out.dtype))
        assert bias is None or bias.dtype == torch.float32
    if GEMM_TIMING is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tstream = torch.cuda.ExternalStream(st) if stream is not None else torch.cuda.current_stream()     # the events go where the launch goes
        e0.record(tstream)
    check(lib.emo_gemm(ptr(A), int(a_trans), _rows(A), ptr(B), int(b_trans), _rows(B), ptr(out), _rows(out), M, N, K,
                       dtype_code(A.dtype), dtype_code(out.dtype), int(accumulate), ctypes.byref(epi), st))
    if GEMM_TIMING is not None:
        e1.record(tstream)
        kind = ('T' if a_trans else 'N') + ('N' if b_trans else 'T')
        fam = lib.emo_gemm_last_kernel() & 15          # the kernel family that RAN (emo_hip.h), not the one the shape suggests
        if fam == 4:
            kind += '/K>1024'
        elif fam == 2:       # one class per kernel INSTANCE (template argument = epilogue flags), as the rocprofv3 summary lists them
            tag = [t for t, on in (('relu', act == ACT_RELU), ('gelu', act == ACT_GELU_NEW), ('drop', p_drop > 0), ('res', residual is not None),
                                   ('bits', mul_mode == MUL_BITMASK), ('mul', mul_aux is not None and mul_mode != MUL_BITMASK), ('mask', mask_out is not None),
                                   ('hdiv', hdiv is not None)) if on]
            kind += '/K=512/' + ('+'.join(tag) if tag else 'plain')
        elif fam == 3:       # 256 x 256 tile wgrad (with / without the bias gradient)
            kind += '/rs' if (a_rowsum is not None or b_rowsum is not None) else '/plain'
        elif kind == 'TN':
            kind += '/128'
        elif fam == 1:
            kind += '/skinny'
        GEMM_TIMING.append((kind, e0, e1, 2.0 * M * N * K,
                            (M * K + N * K) * A.element_size() + M * N * out.element_size(), (M, N, K)))
    if lna is not None:
        return out, ln_out, ln_mean, ln_rstd
    return out


def __getattr__(name):
    if name == 'ASTAT_MIN_ROWS':       # fewest rows of the A-stationary class (128-row panels; below one panel per CU the kernel splits the columns over the grid)
        return lib.emo_gemm_astat_min_rows()
    raise AttributeError(name)


def gemm_astat_ok(M, N, K, in_dtype, out_dtype):
    """The A-stationary K = 512 class of emo_gemm as far as it does not depend on the tensors: the library's own predicate (emo_hip.h)."""
    return in_dtype == torch.bfloat16 and bool(lib.emo_gemm_astat_supported(BF16, dtype_code(out_dtype), M, N, K))


def gemm_bitmask_ok(M, N, K, in_dtype, out_dtype):
    """Shape class in which emo_gemm writes / reads the 1-bit epilogue mask (mask_out / MUL_BITMASK): the A-stationary K = 512 kernel."""
    return out_dtype == torch.bfloat16 and gemm_astat_ok(M, N, K, in_dtype, out_dtype)


def gemm_lna_ok(M, N, K, in_dtype):
    """Shape class in which emo_gemm can take the LayerNorm of its A operand (lna=): the A-stationary K = 512 kernel (emo_hip.h: lna_*).
    Strides / alignment are asserted by gemm() itself, which owns the tensors — lna_* has no other kernel to fall back to."""
    return os.environ.get('EMO_LN_IN_GEMM', '1') != '0' and gemm_astat_ok(M, N, K, in_dtype, in_dtype)


def bitmask_rows(mask, M, N):
    """Row-major view [M, N/8] (byte (m, n/8), bit j = column 8 (n/8) + j) of a mask in emo_gemm's tiled layout (emo_hip.h: mask_out) — tests / diagnostics."""
    t = mask.reshape(M // 32, N // 64, 4, 16, 2, 2)           # [row panel, column tile, g = column group, r = row % 16, i = row / 16, h = column / 32]
    return t.permute(0, 4, 3, 1, 5, 2).reshape(M, N // 8)


def ffn_fwd_ok(M, d_model, d_ff, dtype):
    """True when ffn_fwd serves the problem (emo_hip.h: emo_ffn_fwd — the feed-forward block in one launch)."""
    return dtype == torch.bfloat16 and bool(lib.emo_ffn_fwd_supported(dtype_code(dtype), M, d_model, d_ff))


def ffn_fwd(x1, gamma, beta, W1, b1, W2, b2, p_drop=0.0, seed=0, offset_f=0, offset_y=0, eps=1e-5):
    """(f, h1, mean, rstd, mask, x2) of the fused feed-forward block: h1 = LN(x1), f = drop(relu(h1 W1^T + b1)), x2 = h1 + drop(f W2^T + b2)."""
    M, D = x1.shape
    Hd = W1.shape[0]
    assert x1.is_contiguous() and W1.is_contiguous() and W2.is_contiguous() and W1.shape == (Hd, D) and W2.shape == (D, Hd)
    assert b1.dtype == torch.float32 and b2.dtype == torch.float32 and gamma.dtype == torch.float32 and beta.dtype == torch.float32
    dev, dt = x1.device, x1.dtype
    h1, x2 = torch.empty_like(x1), torch.empty_like(x1)
    f = torch.empty(M, Hd, device=dev, dtype=dt)
    mean, rstd = torch.empty(M, device=dev, dtype=torch.float32), torch.empty(M, device=dev, dtype=torch.float32)
    mask = torch.empty(M, Hd // 8, device=dev, dtype=torch.uint8)
    flops, nbytes = 2.0 * 2.0 * M * D * Hd, (3.0 * M * D + M * Hd) * x1.element_size() + M * Hd / 8
    with _timed('ffn_fused_fwd', flops, nbytes):
        check(lib.emo_ffn_fwd(ptr(x1), ptr(gamma), ptr(beta), eps, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(h1), ptr(mean), ptr(rstd), ptr(f), ptr(mask),
                              ptr(x2), M, D, Hd, dtype_code(dt), p_drop, seed, offset_f, offset_y, stream()))
    return f, h1, mean, rstd, mask, x2


def colsum(X, out=None, accumulate=False):
    M, N = X.shape
    if out is None:
        out = torch.empty(N, device=X.device, dtype=torch.float32)
    check(lib.emo_colsum(ptr(X), dtype_code(X.dtype), M, N, _rows(X), ptr(out), int(accumulate), stream()))
    return out


def embed_fwd(tok, seg, E, S, pe, dtype, scale, pos0=0, p_drop=0.0, seed=0, offset=0, pos_ids=None):
    B, T = tok.shape
    D = E.shape[1]
    out = torch.empty(B, T, D, device=tok.device, dtype=dtype)
    assert pe.is_contiguous() and pe.shape[-1] == D and pe.numel() >= (pos0 + T) * D
    tok, seg, pos_ids = _c(tok), _c(seg), _c(pos_ids)       # keep the contiguous copies alive until the launch is queued
    check(lib.emo_embed_fwd(ptr(tok), ptr(seg), ptr(E), ptr(S), ptr(pe), ptr(out),
                            dtype_code(dtype), B, T, D, E.shape[0], 0 if S is None else S.shape[0], pos0, ptr(pos_ids), scale, p_drop, seed,
                            offset, stream()))
    return out


def embed_bwd(tok, seg, dout, dE, dS, scale, p_drop=0.0, seed=0, offset=0):
    B, T = tok.shape
    D = dE.shape[1]
    assert dout.is_contiguous()
    tok, seg = _c(tok), _c(seg)
    check(lib.emo_embed_bwd(ptr(tok), ptr(seg), ptr(dout), dtype_code(dout.dtype),
                            ptr(dE), ptr(dS), B, T, D, dE.shape[0], 0 if dS is None else dS.shape[0], scale, p_drop, seed, offset,
                            stream()))


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    M, D = x.shape
    assert x.is_contiguous()
    y = torch.empty_like(x)
    mean = torch.empty(M, device=x.device, dtype=torch.float32)
    rstd = torch.empty(M, device=x.device, dtype=torch.float32)
    check(lib.emo_layernorm_fwd(ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), dtype_code(x.dtype), M, D, eps, stream()))
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dres=None, want_drop=False, p_drop=0.0, seed=0, offset=0, dcol=None):
    M, D = x.shape
    assert dy.is_contiguous() and x.is_contiguous() and (dres is None or dres.is_contiguous())
    dx = torch.empty_like(x)
    dxd = torch.empty_like(x) if want_drop else None
    ws, ws_bytes = _workspace('ln_bwd', x.device, lib.emo_layernorm_bwd_workspace_bytes(dtype_code(x.dtype), M, D))
    check(lib.emo_layernorm_bwd(ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(dxd), ptr(dgamma), ptr(dbeta),
                                ptr(dcol), dtype_code(x.dtype), M, D, p_drop, seed, offset, ptr(ws), ws_bytes, stream()))
    return dx, dxd


def dropout_apply(x, p_drop, seed, offset):
    assert x.is_contiguous()
    out = torch.empty_like(x)
    check(lib.emo_dropout_apply(ptr(x), ptr(out), dtype_code(x.dtype), x.numel(), p_drop, seed, offset, stream()))
    return out


def _attn(kind, pass_, q, k, v, B, T, H, **fields):
    """One emo_attn call (emo_hip.h) from a fresh emo_attn_t: the kind, the pass, the q / k / v views ([B*T, H*dh], one row stride; the RELPOS
    BWD_KV / BWD_R passes take their biased query copies as `qu`, `qv` fields and read no q; the DECODE passes of SOFTMAX and RELPOS take
    k = v = None when nothing is appended to the caches) and the shape; every other field by its name in the struct, tensors as ptr(t).  The block
    lives for this call only: the library reads it at call time."""
    assert (k is None) == (v is None)
    ld = _rows(q if k is None else k)
    same_ld = lambda t: _rows(t) == ld or t.shape[0] == 1        # (the stride of a single row is whatever the view left there)
    assert q.shape[0] == B * T and (k is None or same_ld(v)) and (pass_ in (ATTN_BWD_KV, ATTN_BWD_R) or same_ld(q))
    a = Attn(kind=kind, pass_=pass_, q=ptr(q), k=ptr(k), v=ptr(v), ld=ld, dtype=dtype_code(q.dtype), B=B, T=T, H=H, dh=q.shape[1] // H, **fields)
    check(lib.emo_attn(ctypes.byref(a), stream()))


def _favor_workspace(device, B, T, H, dh, n_feat):
    """Scratch for the segment-parallel scan (see include/emo_hip.h)."""
    return _workspace('favor', device, lib.emo_favor_attn_workspace_bytes(B, T, H, dh, n_feat))


def favor_attn_fwd(q, k, v, omega, B, T, H, eps=1e-6, want_state=False, keep_ws=False):
    """q,k,v: [B*T, H*dh] (row-strided views allowed). Returns out [B*T, H*dh], den [B,H,T] (, S, z).
    keep_ws: the call gets a PRIVATE workspace, returned as a third value (None when the scan is not segmented) for favor_attn_bwd(ws_saved=):
    the backward then skips recomputing the K-state increments (include/emo_hip.h, emo_attn_t.kstate_valid)."""
    M, HD = q.shape
    dh = HD // H
    n_feat = 2 * omega.shape[1]
    assert omega.shape[0] == dh and omega.dtype == torch.float32 and omega.is_contiguous()
    out = torch.empty(M, HD, device=q.device, dtype=q.dtype)
    den = torch.empty(B, H, T, device=q.device, dtype=torch.float32)
    S = torch.empty(B, H, n_feat, dh, device=q.device, dtype=torch.float32) if want_state else None
    z = torch.empty(B, H, n_feat, device=q.device, dtype=torch.float32) if want_state else None
    if keep_ws:
        ws_bytes = lib.emo_favor_attn_workspace_bytes(B, T, H, dh, n_feat)
        ws = torch.empty(ws_bytes, device=q.device, dtype=torch.uint8) if ws_bytes else None
    else:
        ws, ws_bytes = _favor_workspace(q.device, B, T, H, dh, n_feat)
    # algorithmic HBM bytes: read q, k, v + write out = 4 * H*dh * e per token
    with _timed('favor_fwd', 0.0, 4.0 * M * HD * q.element_size()):
        _attn(ATTN_FAVOR, ATTN_FWD, q, k, v, B, T, H, omega=ptr(omega), out=ptr(out), ld_out=HD, den=ptr(den), state_S=ptr(S), state_z=ptr(z),
              n_feat=n_feat, eps=eps, workspace=ptr(ws), workspace_bytes=ws_bytes)
    if keep_ws:
        assert not want_state
        return out, den, ws
    return (out, den, S, z) if want_state else (out, den)


def favor_bwd_dn_ok(dtype, B, T, H, dh, n_feat):
    """True when favor_attn_bwd(dn=True) serves the problem (emo_hip.h: emo_attn_t.dout_is_dn — the single-segment slice kernels)."""
    return dtype == torch.bfloat16 and bool(lib.emo_favor_attn_bwd_dn_supported(dtype_code(dtype), B, T, H, dh, n_feat))


def favor_attn_bwd(q, k, v, omega, out, dout, den, B, T, H, dqkv=None, eps=1e-6, ws_saved=None, dn=False):
    """Returns (dq, dk, dv) views of one fused [B*T, 3*H*dh] buffer (ready for the fused-QKV dgrad/wgrad).
    dn=True: `dout` is already dN = dout / den (gemm(hdiv=(den, T)) produced it); den is not read."""
    M, HD = q.shape
    dh = HD // H
    n_feat = 2 * omega.shape[1]
    assert out.is_contiguous() and dout.is_contiguous()
    if dqkv is None:
        dqkv = torch.empty(M, 3 * HD, device=q.device, dtype=q.dtype)
    dq, dk, dv = dqkv[:, :HD], dqkv[:, HD:2 * HD], dqkv[:, 2 * HD:]
    if dn:                                                        # single-segment scan: no workspace either
        ws, ws_bytes, kvalid = None, 0, 0
    elif ws_saved is not None:                                    # the forward's private workspace: its K-state increments are still there
        ws, ws_bytes, kvalid = ws_saved, ws_saved.numel(), 1
        assert ws_bytes == lib.emo_favor_attn_workspace_bytes(B, T, H, dh, n_feat)
    else:
        (ws, ws_bytes), kvalid = _favor_workspace(q.device, B, T, H, dh, n_feat), 0
    # read q, k, v, dout (+ out) + write dq, dk, dv = 7 * H*dh * e per token
    with _timed('favor_bwd', 0.0, 7.0 * M * HD * q.element_size()):
        _attn(ATTN_FAVOR, ATTN_BWD, q, k, v, B, T, H, omega=ptr(omega), out=ptr(out), dout=ptr(dout), ld_out=HD, den=ptr(den),
              dq=ptr(dq), dk=ptr(dk), dv=ptr(dv), ld_d=3 * HD, n_feat=n_feat, eps=eps, workspace=ptr(ws), workspace_bytes=ws_bytes,
              kstate_valid=kvalid, dout_is_dn=int(dn))
    return dq, dk, dv


def favor_decode_step(q, k, v, omega, state_S, state_z, H, eps=1e-6):
    n, HD = q.shape
    out = torch.empty(n, HD, device=q.device, dtype=q.dtype)
    _attn(ATTN_FAVOR, ATTN_DECODE, q, k, v, n, 1, H, omega=ptr(omega), state_S=ptr(state_S), state_z=ptr(state_z), out=ptr(out), ld_out=HD,
          n_feat=2 * omega.shape[1], eps=eps)
    return out


TXL_PARAM_WORDS = TXL_STATE_WORDS = ACC_PARAM_WORDS = ACC_STATE_WORDS = 8     # emo_hip.h: EMO_TXL_* / EMO_ACC_*_WORDS
_F32, _I32, _I64 = torch.float32, torch.int32, torch.int64


def _is(t, dtype):
    return t.dtype == dtype and t.is_contiguous()


# layout a tensor must have before its address goes into a DecodeStep field: field -> check(args, tensor)
_DECODE_STEP_LAYOUT = {
    'logits': lambda a, t: _is(t, _F32) and t.shape == (a.n_streams, a.n_token),
    'ln0': lambda a, t: _is(t, _F32) and t.numel() == 2 * a.d_model,
    'u_steps': lambda a, t: _is(t, _F32) and t.shape[1] == a.n_real,
    'step': lambda a, t: t.dtype == _I64,
    'tok_out': lambda a, t: t.dtype == _I64,
    'seq': lambda a, t: t.dtype == _I64 and t.stride(1) == 1,
    'lens': lambda a, t: t.numel() == a.n_streams,
    'r_w_bias': lambda a, t: _is(t, _F32),
    'r_r_bias': lambda a, t: _is(t, _F32),
}
_DECODE_STEP_I64 = ('tok', 'seg', 'pos_ids', 'lens')          # int64 vectors, made contiguous (_c)
# the same for a GrammarStep, against the numbers of the block: n_rows (n, or the m rows of the windowed batch), n_token, ld_u = the number of
# streams, window (0 outside the windowed kind), and ld_seq, which `seq` sets: hand over seq before segs
_GRAMMAR_STEP_LAYOUT = {
    'logits': lambda a, t: _is(t, _F32) and t.shape == (a.n_rows, a.n_token),
    'u_steps': lambda a, t: _is(t, _F32) and t.dim() == 2 and t.shape[1] == a.ld_u,
    'ev_flags': lambda a, t: _is(t, _I32) and t.numel() >= a.n_token,
    'ev_beat': lambda a, t: _is(t, _I32) and t.numel() >= a.n_token,
    'params': lambda a, t: _is(t, _I32) and t.shape == (a.ld_u, ACC_PARAM_WORDS),
    'state': lambda a, t: _is(t, _I32) and t.shape == (a.ld_u, ACC_STATE_WORDS),
    'running': lambda a, t: _is(t, _I32) and t.numel() >= 1,
    'seq': lambda a, t: _is(t, _I64) and t.dim() == 2 and t.shape[0] == a.ld_u and t.shape[1] >= a.window,
    'segs': lambda a, t: _is(t, _I64) and t.shape == (a.ld_u, a.ld_seq),
    'lead_tok': lambda a, t: _is(t, _I64) and t.numel() >= 1,
    'lead_off': lambda a, t: _is(t, _I32) and t.numel() >= 1,
    'tok_out': lambda a, t: _is(t, _I64) and t.numel() == a.n_rows,
    'seg_out': lambda a, t: _is(t, _I64) and t.numel() == a.n_rows,
    # (values in [0, ld_u): checked by the caller on the host — WindowedLoop._set_rows; the kernel skips a row outside that range)
    'rows': lambda a, t: _is(t, _I32) and t.numel() == a.n_rows,
    'win_tok': lambda a, t: _is(t, _I64) and t.shape == (a.n_rows, a.window),
    'win_seg': lambda a, t: _is(t, _I64) and t.shape == (a.n_rows, a.window),
    # the optional per-token outputs: laid out like seq (hand them over after it)
    'tok_logp': lambda a, t: _is(t, _F32) and t.shape == (a.ld_u, a.ld_seq),
    'tok_rank': lambda a, t: _is(t, _I32) and t.shape == (a.ld_u, a.ld_seq),
    'tok_entropy': lambda a, t: _is(t, _F32) and t.shape == (a.ld_u, a.ld_seq),
    # the queue kind: per slot (n_rows) and per job (ld_u = n_jobs)
    'slot_job': lambda a, t: _is(t, _I32) and t.numel() == a.n_rows,
    'queue_head': lambda a, t: _is(t, _I32) and t.numel() >= 1,
    'mem_lens': lambda a, t: _is(t, _I64) and t.numel() == a.n_rows,
    'job_steps': lambda a, t: _is(t, _I32) and t.numel() == a.ld_u,
    'row_reset': lambda a, t: _is(t, _I32) and t.numel() == a.n_rows,
    # the optional sampling controls: per stream (ld_u) like params; the ban rows hold uint32 words (as int32, bit for bit), n_masks of them,
    # given in the same call (numbers are written first)
    'tok_mask': lambda a, t: _is(t, _I32) and t.shape == (a.n_masks, (a.n_token + 31) // 32) and a.n_masks > 0,
    # (the values are read back once, when the table enters the block: a row outside [-1, n_masks) is refused here; the kernel would treat it as -1)
    'mask_of': lambda a, t: _is(t, _I32) and t.numel() == a.ld_u and int(t.min()) >= -1 and int(t.max()) < a.n_masks,
    'temp_of': lambda a, t: _is(t, _F32) and t.numel() == a.ld_u,
    'top_p_of': lambda a, t: _is(t, _F32) and t.numel() == a.ld_u,
    # the optional soft controls, per stream like the four above: shared bias rows (n_biases of them, given in the same call; values finite or
    # -inf, read back once like mask_of's), the row each stream draws under (-1: none), the rank cap and the floor
    'tok_bias': lambda a, t: _is(t, _F32) and t.shape == (a.n_biases, a.n_token) and a.n_biases > 0 and not bool((torch.isnan(t) | (t == float('inf'))).any()),
    'bias_of': lambda a, t: _is(t, _I32) and t.numel() == a.ld_u and int(t.min()) >= -1 and int(t.max()) < a.n_biases,
    'top_k_of': lambda a, t: _is(t, _I32) and t.numel() == a.ld_u,
    'min_p_of': lambda a, t: _is(t, _F32) and t.numel() == a.ld_u and not bool(torch.isnan(t).any()),
    # kinds ACC and TXL, classifier-free guidance: per row of the batch; what the three hold together is checked by _check_guidance once they are in
    'guide_cond': lambda a, t: _is(t, _I32) and t.numel() == a.n_rows,
    'guide_uncond': lambda a, t: _is(t, _I32) and t.numel() == a.n_rows,
    'guide_scale': lambda a, t: _is(t, _F32) and t.numel() == a.n_rows,
    # kinds ACC / ACC_QUEUE, kept bars: keep_beg / keep_end are indexed like lead_off (hand them over after it, and n_keep in the same call or
    # before); what the three hold together is checked by _check_keep once they are in
    'keep_tok': lambda a, t: _is(t, _I64) and t.numel() >= max(a.n_keep, 1),
    'keep_beg': lambda a, t: _is(t, _I32),
    'keep_end': lambda a, t: _is(t, _I32),
    # kinds TXL / TXL_QUEUE, kept bars: the three tables above, indexed by params[KEEP0] + bar (hand them over with or after params), and the
    # per-stream count of kept tokens not yet fed
    'keep_left': lambda a, t: _is(t, _I32) and t.numel() == a.ld_u,
}
_GUIDE = ('guide_cond', 'guide_uncond', 'guide_scale')
_KEEP = ('keep_tok', 'keep_beg', 'keep_end')
_KEEP_TXL = _KEEP + ('keep_left',)
TXL_P_KEEP0, TXL_P_KEEP_BARS = 6, 7                            # emo_hip.h: EMO_TXL_P_KEEP0 / EMO_TXL_P_KEEP_BARS


def guide_pairs_error(c, g, s):
    """The rule of the three guidance tables (lists of equal length n: guide_cond, guide_uncond, guide_scale) -> None, or what is wrong with
    them.  Row r holds (-1, -1) (unguided) or a pair (c, g) of two distinct rows, r one of them, whose other row holds the same pair and the
    same scale; every scale is finite and >= 0."""
    n = len(c)
    if not (len(g) == n and len(s) == n):
        return 'guide tables of %d / %d / %d rows' % (n, len(g), len(s))
    for r in range(n):
        if not (s[r] >= 0 and s[r] != float('inf')):             # (NaN fails the first)
            return 'guide_scale[%d] = %r is not a finite scale >= 0' % (r, s[r])
        if c[r] == -1 and g[r] == -1:
            continue
        if not (0 <= c[r] < n and 0 <= g[r] < n):
            return 'guide pair (%d, %d) of row %d is outside [0, %d)' % (c[r], g[r], r, n)
        if c[r] == g[r]:
            return 'guide pair (%d, %d) of row %d names one row twice' % (c[r], g[r], r)
        if r not in (c[r], g[r]):
            return 'row %d is neither row of its guide pair (%d, %d)' % (r, c[r], g[r])
        o = g[r] if r == c[r] else c[r]
        if (c[o], g[o]) != (c[r], g[r]) or s[o] != s[r]:
            return 'rows %d and %d of a guide pair disagree: (%d, %d) x %r against (%d, %d) x %r' % (r, o, c[r], g[r], s[r], c[o], g[o], s[o])
    return None


def _check_guidance(args, held):
    """The three guidance tables of a GrammarStep as they stand in `held` (read back once, when one of them enters the block, as mask_of is):
    all three or none, and guide_pairs_error's rule.  The kernel reads nothing out of bounds whatever they hold (any other pair is unguided to
    it): these are the checks the launch cannot make."""
    cond, unc, scale = (held.get(k) for k in _GUIDE)
    if cond is None and unc is None and scale is None:
        return
    assert cond is not None and unc is not None and scale is not None, 'grammar step: guide_cond, guide_uncond and guide_scale come together or not at all'
    bad = guide_pairs_error(cond.tolist(), unc.tolist(), scale.tolist())
    assert bad is None, 'grammar step: ' + bad


def _check_keep(args, held):
    """The three kept-bar tables of a GrammarStep as they stand in `held` (read back once, when one of them enters the block): all three or
    none, keep_beg / keep_end as long as lead_off, and every kept range inside keep_tok's n_keep entries.  The kernel reads nothing out of
    bounds whatever they hold (such a range ends its stream OVERFLOW)."""
    if args.kind in (GRAMMAR_TXL, GRAMMAR_TXL_QUEUE):
        return _check_keep_txl(args, held)
    tok, beg, end = (held.get(k) for k in _KEEP)
    if tok is None and beg is None and end is None:
        return
    assert tok is not None and beg is not None and end is not None, 'grammar step: keep_tok, keep_beg and keep_end come together or not at all'
    off = held.get('lead_off')
    assert off is not None and beg.numel() == off.numel() and end.numel() == off.numel(), \
        'grammar step: keep_beg and keep_end have one entry per entry of lead_off'
    b, e = beg.cpu().numpy(), end.cpu().numpy()
    kept = b >= 0
    assert 0 <= args.n_keep <= tok.numel() and bool((e[kept] >= b[kept]).all()) and bool((e[kept] <= args.n_keep).all()), \
        'grammar step: a kept bar lies outside keep_tok[0 .. n_keep)'


def _check_keep_txl(args, held):
    """The same for kinds TXL / TXL_QUEUE (messages name the kind): keep_tok, keep_beg, keep_end and keep_left all four or none; keep_beg and
    keep_end of one length that holds every stream's params[KEEP0] .. KEEP0 + params[KEEP_BARS]; every kept range inside keep_tok's n_keep
    entries; keep_left within [0, ld_seq]."""
    who = 'grammar step[%s]' % ('txl' if args.kind == GRAMMAR_TXL else 'txl_queue')
    tok, beg, end, left = (held.get(k) for k in _KEEP_TXL)
    if tok is None and beg is None and end is None and left is None:
        return
    assert tok is not None and beg is not None and end is not None and left is not None, \
        who + ': keep_tok, keep_beg, keep_end and keep_left come together or not at all'
    assert beg.numel() == end.numel(), who + ': keep_beg and keep_end have one length'
    assert 0 <= args.keep_bar < args.n_token, who + ': keep_bar = %d lies outside [0, %d)' % (args.keep_bar, args.n_token)
    params = held.get('params')
    assert params is not None, who + ': the kept-bar tables are indexed by params: hand them over with it or after it'
    p = params.cpu().numpy()
    k0, kn = p[:, TXL_P_KEEP0].astype('int64'), p[:, TXL_P_KEEP_BARS].astype('int64')
    assert bool((k0 >= 0).all()) and bool((kn >= 0).all()) and bool((k0 + kn <= beg.numel()).all()), \
        who + ': params[KEEP0] .. KEEP0 + params[KEEP_BARS] lies outside keep_beg / keep_end'
    b, e = beg.cpu().numpy(), end.cpu().numpy()
    kept = b >= 0
    assert 0 <= args.n_keep <= tok.numel() and bool((e[kept] >= b[kept]).all()) and bool((e[kept] <= args.n_keep).all()), \
        who + ': a kept bar lies outside keep_tok[0 .. n_keep)'
    lf = left.cpu().numpy()
    assert bool((lf >= 0).all()) and bool((lf <= args.ld_seq).all()), who + ': keep_left lies outside [0, ld_seq]'


# per struct: its name in messages, the layout table, the int64 vectors, and the numbers a tensor brings with it (field -> (number, of tensor))
_BLOCKS = {
    DecodeStep: ('decode step', _DECODE_STEP_LAYOUT, _DECODE_STEP_I64,
                 {'seq': ('ld_seq', lambda t: t.stride(0)), 'sync_ws': ('sync_ws_bytes', lambda t: t.numel() * t.element_size())}),
    GrammarStep: ('grammar step', _GRAMMAR_STEP_LAYOUT, (),
                  {'seq': ('ld_seq', lambda t: t.shape[1]), 'u_steps': ('n_u', lambda t: t.shape[0])}),
}


def block_set(args, held, **fields):
    """Write fields of an argument block, a DecodeStep or a GrammarStep (emo_hip.h: emo_decode_step_t, emo_grammar_step_t): numbers as they are,
    tensors (or None) as device addresses after the layout check of the field in the struct's table; a tensor that brings a number with it sets
    that too (`seq` ld_seq; DecodeStep `sync_ws` sync_ws_bytes; GrammarStep `u_steps` n_u); the three guidance tables of a GrammarStep are given
    in one call and checked together (_check_guidance).  The struct holds raw addresses, so the rule of _c()
    applies to its owner: `held` (field -> tensor) is the owner's dict that keeps every tensor whose address is in the struct alive, the
    contiguous copies made here included.  A tensor that `held` already has for the field is the one the struct points to, checked when it went
    in: it is not looked at again (a token loop hands over the same buffers step after step).  Numbers are written first: a tensor may be
    checked against a size given in the same call."""
    what, layout, i64, brings = _BLOCKS[type(args)]
    tensors = None
    for k, v in fields.items():
        if v is None or isinstance(v, torch.Tensor):
            if k not in held or held[k] is not v:
                tensors = tensors or []
                tensors.append((k, v))
        else:
            setattr(args, k, v)
    for k, t in tensors or ():
        if t is not None:
            if k in i64:
                t = _c(t)                                         # (a copy is held in the caller's place, so the next call makes a new one)
            ok = layout.get(k)
            assert ok is None or ok(args, t), '%s: bad dtype / layout of %s' % (what, k)
        held[k] = t
        setattr(args, k, ptr(t))
        if k in brings:
            number, of = brings[k]
            setattr(args, number, 0 if t is None else of(t))
    if tensors and type(args) is GrammarStep and any(k in _GUIDE for k, _ in tensors):
        try:
            _check_guidance(args, held)
        except AssertionError:
            for k in _GUIDE:                                      # a refused set never stays in the block
                held.pop(k, None)
                setattr(args, k, None)
            raise
    # (kinds TXL / TXL_QUEUE index keep_beg / keep_end by words of params: a new params is checked against the tables the block holds)
    if tensors and type(args) is GrammarStep and any(k in _KEEP_TXL or k == 'params' for k, _ in tensors):
        try:
            _check_keep(args, held)
        except AssertionError:
            for k in _KEEP_TXL:
                held.pop(k, None)
                setattr(args, k, None)
            raise


decode_step_set = block_set


def decode_step(args):
    """One token step of every stream in ONE persistent launch (emo_hip.h: emo_decode_step) from a prepared DecodeStep; its logits field is the output."""
    check(lib.emo_decode_step(ctypes.byref(args), stream()))


def favor_draw_omega(gauss, omega):
    """gauss [L, nb, dh, dh] ~ N(0,1) -> omega [L, dh, n_feat/2] (orthogonal blocks scaled by row norms)."""
    L, nb, dh, _ = gauss.shape
    assert gauss.is_contiguous() and omega.is_contiguous() and omega.shape[:2] == (L, dh)
    check(lib.emo_favor_draw_omega(ptr(gauss), ptr(omega), L, dh, 2 * omega.shape[2], stream()))
    return omega


def favor_state_reset(state_table, n_rows, s_row_floats, z_row_floats, row_reset):
    """Zero the FAVOR+ state rows flagged in row_reset (int32 [n_rows]; emo_hip.h: emo_favor_state_reset).  state_table: int64 [n_layers, 2] on the
    device, the data_ptr() of every layer's S [n_rows, H, F, dh] and z [n_rows, H, F] (fp32, contiguous; the caller keeps them alive).
    Allocation-free (hipGraph capture)."""
    assert state_table.dtype == _I64 and state_table.is_contiguous() and state_table.dim() == 2 and state_table.shape[1] == 2
    assert _is(row_reset, _I32) and row_reset.numel() == n_rows
    check(lib.emo_favor_state_reset(ptr(state_table), state_table.shape[0], n_rows, s_row_floats, z_row_floats, ptr(row_reset), stream()))


def favor_state_at(k, v, omega, lens, B, T, H, out=None):
    """The FAVOR+ recurrent state of every row at its own length (emo_hip.h: emo_favor_state_at).  k, v: [B*T, H*dh] (row-strided views allowed),
    lens int32 [B] on the device, 1 <= lens[b] <= T -> (S f32 [B, H, n_feat, dh], z f32 [B, H, n_feat]); out = (S, z): written in place.
    Allocation-free with `out`."""
    HD = k.shape[1]
    dh, n_feat = HD // H, 2 * omega.shape[1]
    assert k.shape == v.shape and k.shape[0] == B * T and k.dtype == v.dtype and _rows(k) == _rows(v)
    assert omega.shape[0] == dh and omega.dtype == _F32 and omega.is_contiguous()
    assert _is(lens, _I32) and lens.numel() == B
    if out is None:
        out = (torch.empty(B, H, n_feat, dh, device=k.device, dtype=_F32), torch.empty(B, H, n_feat, device=k.device, dtype=_F32))
    S, z = out
    assert _is(S, _F32) and S.shape == (B, H, n_feat, dh) and _is(z, _F32) and z.shape == (B, H, n_feat)
    check(lib.emo_favor_state_at(ptr(k), ptr(v), _rows(k), dtype_code(k.dtype), ptr(omega), ptr(lens), ptr(S), ptr(z), B, T, H, dh, n_feat, stream()))
    return S, z


def softmax_attn_fwd(q, k, v, B, T, H, p_drop=0.0, seed=0, offset=0, want_keep=False):
    """want_keep: also return the dropout keep words for softmax_attn_bwd (None when the call has none: include/emo_hip.h)."""
    M, HD = q.shape
    dh = HD // H
    out = torch.empty(M, HD, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, H, T, device=q.device, dtype=torch.float32)
    keep, kbytes = None, 0
    if want_keep and all(t.data_ptr() % 16 == 0 for t in (q, k, v)):
        kbytes = lib.emo_softmax_attn_keep_bytes(dtype_code(q.dtype), B, T, H, dh, p_drop)
        if kbytes:
            keep = torch.empty(kbytes // 4, device=q.device, dtype=torch.int32)
    # 2 matmuls (Q K^T, P V) of 2*T*T*dh FLOP per (b, h), half of the tiles skipped by the causal mask
    with _timed('sattn_fwd', 0.5 * 2 * 2.0 * B * H * T * T * dh, 4.0 * M * HD * q.element_size()):
        _attn(ATTN_SOFTMAX, ATTN_FWD, q, k, v, B, T, H, out=ptr(out), ld_out=HD, lse=ptr(lse), p_drop=p_drop, seed=seed, offset=offset,
              keep=ptr(keep), keep_bytes=kbytes)
    return (out, lse, keep) if want_keep else (out, lse)


def softmax_attn_bwd(q, k, v, out, dout, lse, B, T, H, p_drop=0.0, seed=0, offset=0, dqkv=None, keep=None):
    M, HD = q.shape
    dh = HD // H
    assert out.is_contiguous() and dout.is_contiguous()
    if dqkv is None:
        dqkv = torch.empty(M, 3 * HD, device=q.device, dtype=q.dtype)
    dq, dk, dv = dqkv[:, :HD], dqkv[:, HD:2 * HD], dqkv[:, 2 * HD:]
    delta = torch.empty(B, H, T, device=q.device, dtype=torch.float32)          # dO.O per query row, handed from the dQ to the dK/dV pass
    # dQ pass: S, dP, dQ; dK/dV pass: S, dP, dV, dK = 7 matmuls, causal half
    with _timed('sattn_bwd', 0.5 * 7 * 2.0 * B * H * T * T * dh, 8.0 * M * HD * q.element_size()):
        _attn(ATTN_SOFTMAX, ATTN_BWD, q, k, v, B, T, H, out=ptr(out), dout=ptr(dout), ld_out=HD, lse=ptr(lse), delta_ws=ptr(delta), dq=ptr(dq),
              dk=ptr(dk), dv=ptr(dv), ld_d=3 * HD, p_drop=p_drop, seed=seed, offset=offset, keep=ptr(keep),
              keep_bytes=0 if keep is None else keep.numel() * 4)
    return dq, dk, dv


def softmax_attn_decode(q, kcache, vcache, lens, H, lens_off=0, k_new=None, v_new=None):
    """One query row per stream against the KV caches; k_new / v_new: the new token's rows, appended in-kernel at position lens + lens_off - 1.
    Caches: [n, T_max, H * dh], or head-major [n, H, T_max, dh] (4-D tensors)."""
    n, HD = q.shape
    head_major = kcache.dim() == 4
    T_max = kcache.shape[2] if head_major else kcache.shape[1]
    assert kcache.is_contiguous() and vcache.is_contiguous() and lens.dtype == torch.int64 and kcache.shape == vcache.shape
    assert not head_major or (kcache.shape[1] == H and kcache.shape[3] == HD // H)
    out = torch.empty(n, HD, device=q.device, dtype=q.dtype)
    _attn(ATTN_SOFTMAX, ATTN_DECODE, q, k_new, v_new, n, 1, H, kcache=ptr(kcache), vcache=ptr(vcache), T_max=T_max, lens=ptr(lens), lens_off=lens_off,
          head_major=int(head_major), out=ptr(out), ld_out=HD)
    return out


def relpos_attn_fwd(q, k, v, r_dist, r_w_bias, r_r_bias, B, T, H, p_drop=0.0, seed=0, offset=0, window=0):
    """Transformer-XL relative-position causal attention (stage 1).  q,k,v [B*T, H*dh] views; r_dist [>=T, H*dh] indexed by distance.
    window = W > 0 (evaluation, p_drop = 0): query i sees keys max(0, i - W) .. i, the window of relpos_attn_decode with mem_len = W; r_dist
    then needs min(T, W + 1) rows (the library checks it)."""
    M, HD = q.shape
    assert r_dist.dtype == q.dtype and (window > 0 or r_dist.shape[0] >= T)
    assert r_w_bias.dtype == torch.float32 and r_r_bias.dtype == torch.float32 and r_w_bias.is_contiguous() and r_r_bias.is_contiguous()
    out = torch.empty(M, HD, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, H, T, device=q.device, dtype=torch.float32)
    zden = torch.empty(B, H, T, device=q.device, dtype=torch.float32)
    _attn(ATTN_RELPOS, ATTN_FWD, q, k, v, B, T, H, r_dist=ptr(r_dist), ld_r=_rows(r_dist), n_dist=r_dist.shape[0], r_w_bias=ptr(r_w_bias),
          r_r_bias=ptr(r_r_bias), out=ptr(out), ld_out=HD, lse=ptr(lse), zden=ptr(zden), p_drop=p_drop, seed=seed, offset=offset, window=int(window))
    return out, lse, zden


def relpos_attn_bwd(qkv, r_dist, r_w_bias, r_r_bias, out, dout, lse, zden, B, T, H, p_drop=0.0, seed=0, offset=0, acc_dq=None, acc_rr=None, dR_out=None, dq_rel_out=None):
    """Backward of relpos_attn_fwd.  qkv [B*T, 3*H*dh] (the fused projection).  Returns dqkv [B*T, 3*H*dh], dR [T, H*dh] fp32 (gradient of
    r_dist rows 0..T-1), d r_w_bias [H, dh], d r_r_bias [H, dh] fp32.  Three kernels, each recomputing the probabilities of its tiles:
    query-tile pass (dq = content + relative part), key-tile pass (dk, dv), distance-window pass (dR) — include/emo_hip.h."""
    M, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    dt, dev = qkv.dtype, qkv.device
    assert M == B * T and out.is_contiguous() and dout.is_contiguous() and qkv.is_contiguous()
    dqkv = torch.empty(M, D3, device=dev, dtype=dt)
    # dq_rel_out: caller's [M, D] buffer for the relative part of dq (the training stack keeps all layers' in one tensor and takes ONE column sum)
    dq_rel = dq_rel_out if dq_rel_out is not None else torch.empty(M, D, device=dev, dtype=dt)
    assert dq_rel.shape == (M, D) and dq_rel.dtype == dt and dq_rel.is_contiguous()
    delta = torch.empty(B, H, T, device=dev, dtype=torch.float32)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    # what the three passes share: r_dist, the incoming gradient, the saved statistics and the dropout stream
    common = dict(r_dist=ptr(r_dist), ld_r=_rows(r_dist), n_dist=r_dist.shape[0], dout=ptr(dout), ld_out=D, lse=ptr(lse), zden=ptr(zden), delta=ptr(delta),
                  ld_d=D3, p_drop=p_drop, seed=seed, offset=offset)
    _attn(ATTN_RELPOS, ATTN_BWD, q, k, v, B, T, H, r_w_bias=ptr(r_w_bias), r_r_bias=ptr(r_r_bias), out=ptr(out), dq=ptr(dqkv), dq_rel=ptr(dq_rel), ld_rel=D,
          **common)
    if acc_rr is not None:                                      # training stack: column sums accumulated over the layers, no per-layer ATen ops —
        if acc_dq is not None:                                  # acc_dq += colsum(dq) (None: the caller takes it from the qkv_net weight-gradient
            colsum(dqkv[:, :D], out=acc_dq, accumulate=True)    # GEMM's a_rowsum, one launch fewer), acc_rr += colsum(dq_rel); the caller forms
        if dq_rel_out is None:
            colsum(dq_rel, out=acc_rr, accumulate=True)         # d r_r_bias = acc_rr, d r_w_bias = acc_dq - acc_rr once per backward
        d_rr = d_rw = None
    else:
        d_rr = colsum(dq_rel)                                   # sum over (b, i) of the relative part of dq = d r_r_bias
        d_rw = (colsum(dqkv[:, :D]) - d_rr).view(H, dh)         # ... of the content part = d r_w_bias
        d_rr = d_rr.view(H, dh)
    qu, qv = add_bias2(q, r_w_bias, r_r_bias)                   # q + r_w_bias, q + r_r_bias
    common.update(qu=ptr(qu), qv=ptr(qv), ld_q=D)
    _attn(ATTN_RELPOS, ATTN_BWD_KV, qu, k, v, B, T, H, dk=ptr(dqkv[:, D:2 * D]), dv=ptr(dqkv[:, 2 * D:]), **common)
    if dR_out is not None:                                      # caller's fp32 [>= T, D] view (row-strided: one column block of a buffer shared by all layers)
        assert dR_out.dtype == torch.float32 and dR_out.shape[1] == D and dR_out.shape[0] >= T and dR_out.stride(1) == 1
        dR = dR_out
    else:
        dR = torch.empty(T, D, device=dev, dtype=torch.float32)
    ws, ws_bytes = _workspace('relpos_dr', dev, lib.emo_relpos_attn_bwd_r_workspace_bytes(B, T, H, dh))
    _attn(ATTN_RELPOS, ATTN_BWD_R, qu, k, v, B, T, H, dR=ptr(dR), ld_dr=_rows(dR), workspace=ptr(ws), workspace_bytes=ws_bytes, **common)
    return dqkv, dR, d_rw, d_rr


def relpos_attn_decode(q, kcache, vcache, lens, H, r_dist, r_w_bias, r_r_bias, mem_len=0, lens_off=0, k_new=None, v_new=None):
    n, HD = q.shape
    T_max = kcache.shape[1]
    assert kcache.is_contiguous() and vcache.is_contiguous() and lens.dtype == torch.int64 and r_dist.shape[0] >= T_max
    out = torch.empty(n, HD, device=q.device, dtype=q.dtype)
    _attn(ATTN_RELPOS, ATTN_DECODE, q, k_new, v_new, n, 1, H, kcache=ptr(kcache), vcache=ptr(vcache), T_max=T_max, lens=ptr(lens), lens_off=lens_off,
          window=mem_len, r_dist=ptr(r_dist), ld_r=_rows(r_dist), n_dist=r_dist.shape[0], r_w_bias=ptr(r_w_bias), r_r_bias=ptr(r_r_bias), out=ptr(out),
          ld_out=HD)
    return out


def xent_fwd(logits, tgt, ignore_index):
    M, V = logits.shape
    assert logits.is_contiguous() and logits.dtype == torch.float32
    lse = torch.empty(M, device=logits.device, dtype=torch.float32)
    acc = torch.zeros(2, device=logits.device, dtype=torch.float32)
    tgt = _c(tgt)
    check(lib.emo_xent_fwd(ptr(logits), ptr(tgt), M, V, ignore_index, ptr(lse), ptr(acc), stream()))
    return lse, acc


def xent_bwd(logits, tgt, lse, gscale, ignore_index, out_dtype, ld_out=None):
    M, V = logits.shape
    ld_out = ld_out or ((V + 7) // 8) * 8
    dl = torch.empty(M, ld_out, device=logits.device, dtype=out_dtype)
    tgt = _c(tgt)
    check(lib.emo_xent_bwd(ptr(logits), ptr(tgt), ptr(lse), ptr(gscale), ptr(dl), ld_out, dtype_code(out_dtype), M, V,
                           ignore_index, stream()))
    return dl


def token_scores(logits, tgt, ignore_index, V=None, want=('lse', 'rank', 'entropy')):
    """Per-row cross-entropy terms of fp32 logits [M, ld] (row-strided views allowed; only columns < V are read, V defaults to the width):
    dict with 'nll' (0 on ignored rows) and whichever of 'lse', 'rank' (int32, -1 on ignored rows), 'entropy' `want` names."""
    assert logits.dtype == torch.float32
    M, ld = logits.shape[0], _rows(logits)
    V = logits.shape[1] if V is None else V
    assert 0 < V <= logits.shape[1] and tgt.numel() == M
    unknown = set(want) - {'nll', 'lse', 'rank', 'entropy'}
    if unknown:
        raise ValueError('token_scores: unknown output(s) %s' % sorted(unknown))
    tgt = _c(tgt.reshape(-1))
    out = {'nll': torch.empty(M, device=logits.device, dtype=torch.float32)}
    for name in ('lse', 'rank', 'entropy'):
        if name in want:
            out[name] = torch.empty(M, device=logits.device, dtype=torch.int32 if name == 'rank' else torch.float32)
    check(lib.emo_token_scores(ptr(logits), ld, ptr(tgt), M, V, ignore_index, ptr(out['nll']), ptr(out.get('lse')), ptr(out.get('rank')),
                               ptr(out.get('entropy')), stream()))
    return out


def xent_bwd_rows(logits, tgt, lse, grow, ignore_index, out_dtype, V=None, ld_out=None):
    """xent_bwd with one upstream gradient per row (grow: fp32 [M]); logits as in token_scores."""
    assert logits.dtype == torch.float32 and grow.dtype == torch.float32 and lse.dtype == torch.float32
    M, ld = logits.shape[0], _rows(logits)
    V = logits.shape[1] if V is None else V
    assert 0 < V <= logits.shape[1] and tgt.numel() == M and grow.numel() == M and lse.numel() == M
    ld_out = ld_out or ((V + 7) // 8) * 8
    dl = torch.empty(M, ld_out, device=logits.device, dtype=out_dtype)
    tgt = _c(tgt.reshape(-1))
    grow = grow if grow.is_contiguous() else grow.contiguous()
    check(lib.emo_xent_bwd_rows(ptr(logits), ld, ptr(tgt), ptr(lse), ptr(grow), ptr(dl), ld_out, dtype_code(out_dtype), M, V,
                                ignore_index, stream()))
    return dl


def argmax(logits):
    rows, V = logits.shape
    assert logits.is_contiguous() and logits.dtype == torch.float32
    out = torch.empty(rows, device=logits.device, dtype=torch.int64)
    check(lib.emo_argmax(ptr(logits), rows, V, ptr(out), stream()))
    return out


def sample_nucleus(logits, temperature, top_p, u):
    rows, V = logits.shape
    assert logits.is_contiguous() and logits.dtype == torch.float32 and u.dtype == torch.float32 and u.numel() == rows
    out = torch.empty(rows, device=logits.device, dtype=torch.int64)
    check(lib.emo_sample_nucleus(ptr(logits), rows, V, temperature, top_p, ptr(u), ptr(out), stream()))
    return out


def sample_nucleus_step(logits, temperature, top_p, u_steps, step, seq=None, col0=0, out=None):
    """One lock-step sampling step with device-side loop state (see include/emo_hip.h): uses u_steps[step[r], r], writes the id to out[r]
    and seq[r, col0 + step[r]], increments step[r].  Allocation-free when `out` is given (hipGraph capture)."""
    rows, V = logits.shape
    assert logits.is_contiguous() and logits.dtype == torch.float32 and u_steps.dtype == torch.float32 and u_steps.is_contiguous()
    assert u_steps.shape[-1] == rows and step.dtype == torch.int64 and step.numel() == rows
    assert seq is None or (seq.dtype == torch.int64 and seq.stride(1) == 1 and seq.shape[0] == rows)
    if out is None:
        out = torch.empty(rows, device=logits.device, dtype=torch.int64)
    check(lib.emo_sample_nucleus_step(ptr(logits), rows, V, temperature, top_p, ptr(u_steps), ptr(step), ptr(seq), 0 if seq is None else seq.stride(0),
                                      col0, ptr(out), stream()))
    return out


def grammar_step(args):
    """One device grammar step (emo_hip.h: emo_grammar_step) from a prepared GrammarStep.  Allocation-free (hipGraph capture); the state, token
    and output tensors of the block are updated in place."""
    check(lib.emo_grammar_step(ctypes.byref(args), stream()))


def _grammar_once(kind, **fields):
    """The one-shot form: a fresh block through block_set (every layout check), one call."""
    args = GrammarStep(kind=kind)
    block_set(args, {}, **fields)
    grammar_step(args)


def draw_score_tables(seq):
    """The three optional outputs of a grammar step for the token rows `seq` [n, W], pre-filled with the sentinels a reader tells given tokens
    from drawn ones by: {'tok_logp': NaN fp32, 'tok_rank': -1 int32, 'tok_entropy': NaN fp32}, each [n, W] (the GrammarStep field names)."""
    n, W = seq.shape
    return {'tok_logp': torch.full((n, W), float('nan'), dtype=_F32, device=seq.device),
            'tok_rank': torch.full((n, W), -1, dtype=_I32, device=seq.device),
            'tok_entropy': torch.full((n, W), float('nan'), dtype=_F32, device=seq.device)}


def txl_grammar_step(logits, temperature, top_p, key_temperature, key_top_p, u_steps, ev_flags, ev_beat, params, state, seq, tok_out, running,
                     tok_logp=None, tok_rank=None, tok_entropy=None, guide_cond=None, guide_uncond=None, guide_scale=None):
    """One stage-1 sample-and-grammar step of n streams (include/emo_hip.h, EMO_GRAMMAR_TXL): logits fp32 [n, V], u_steps fp32 [n_u, n],
    ev_flags / ev_beat int32 [V], params / state int32 [n, 8], seq int64 [n, W], tok_out int64 [n], running int32 [1].  state, seq, tok_out
    and running are updated in place.  tok_logp / tok_entropy fp32, tok_rank int32 [n, W] (each optional): the figures of every accepted draw
    at its token's cell (draw_score_tables makes and pre-fills them).  guide_cond / guide_uncond / guide_scale: as in acc_grammar_step."""
    n, V = logits.shape
    _grammar_once(GRAMMAR_TXL, n_rows=n, n_token=V, ld_u=n, temperature=temperature, top_p=top_p, key_temperature=key_temperature,
                  key_top_p=key_top_p, logits=logits, u_steps=u_steps, ev_flags=ev_flags, ev_beat=ev_beat, params=params, state=state, seq=seq,
                  tok_out=tok_out, running=running, tok_logp=tok_logp, tok_rank=tok_rank, tok_entropy=tok_entropy, guide_cond=guide_cond,
                  guide_uncond=guide_uncond, guide_scale=guide_scale)
    return tok_out


def txl_queue_step(logits, temperature, top_p, key_temperature, key_top_p, u_steps, ev_flags, ev_beat, params, state, seq, tok_out, running,
                   slot_job, queue_head, mem_lens, mem_rows, job_steps=None, tok_logp=None, tok_rank=None, tok_entropy=None):
    """One stage-1 sample-and-grammar step of `slots` batch rows working through a queue of n_jobs jobs (include/emo_hip.h,
    EMO_GRAMMAR_TXL_QUEUE): logits fp32 [slots, V], tok_out int64 [slots], slot_job int32 [slots] (-1: free), mem_lens int64 [slots] (the
    model memory's per-row lengths), queue_head int32 [1]; u_steps fp32 [n_u, n_jobs], params / state int32 [n_jobs, 8], seq int64 [n_jobs, W]
    and the optional tables (job_steps int32 [n_jobs]; the score tables [n_jobs, W]) are the jobs'.  Everything but logits, u_steps, params
    and the event tables is updated in place."""
    slots, V = logits.shape
    n_jobs = params.shape[0]
    _grammar_once(GRAMMAR_TXL_QUEUE, n_rows=slots, n_token=V, ld_u=n_jobs, n_jobs=n_jobs, mem_rows=mem_rows, temperature=temperature, top_p=top_p,
                  key_temperature=key_temperature, key_top_p=key_top_p, logits=logits, u_steps=u_steps, ev_flags=ev_flags, ev_beat=ev_beat,
                  params=params, state=state, seq=seq, tok_out=tok_out, running=running, slot_job=slot_job, queue_head=queue_head,
                  mem_lens=mem_lens, job_steps=job_steps, tok_logp=tok_logp, tok_rank=tok_rank, tok_entropy=tok_entropy)
    return tok_out


def acc_grammar_step(logits, temperature, top_p, u_steps, ev_flags, ev_beat, lead_tok, lead_off, params, state, seq, segs, max_len, track_full, pad,
                     tok_out, seg_out, running, tok_logp=None, tok_rank=None, tok_entropy=None, guide_cond=None, guide_uncond=None, guide_scale=None):
    """One stage-2 sample-and-grammar step of n streams (include/emo_hip.h, EMO_GRAMMAR_ACC): logits fp32 [n, V], u_steps fp32 [n_u, n],
    ev_flags / ev_beat int32 [V], lead_tok int64 (flat), lead_off int32, params / state int32 [n, 8], seq / segs int64 [n, W], tok_out / seg_out
    int64 [n], running int32 [1].  state, seq, segs, tok_out, seg_out and running are updated in place.  tok_logp / tok_rank / tok_entropy:
    as in txl_grammar_step.  guide_cond / guide_uncond int32 [n], guide_scale fp32 [n] (all three or none): classifier-free guidance over
    mirrored pairs of streams (emo_hip.h)."""
    n, V = logits.shape
    _grammar_once(GRAMMAR_ACC, n_rows=n, n_token=V, ld_u=n, temperature=temperature, top_p=top_p, max_len=max_len, track_full=track_full, pad=pad,
                  logits=logits, u_steps=u_steps, ev_flags=ev_flags, ev_beat=ev_beat, lead_tok=lead_tok, lead_off=lead_off, params=params, state=state,
                  seq=seq, segs=segs, tok_out=tok_out, seg_out=seg_out, running=running, tok_logp=tok_logp, tok_rank=tok_rank,
                  tok_entropy=tok_entropy, guide_cond=guide_cond, guide_uncond=guide_uncond, guide_scale=guide_scale)
    return tok_out


def acc_queue_step(logits, temperature, top_p, u_steps, ev_flags, ev_beat, lead_tok, lead_off, params, state, seq, segs, max_len, track_full, pad,
                   tok_out, seg_out, running, slot_job, queue_head, mem_lens, mem_rows, row_reset, job_steps=None, tok_logp=None, tok_rank=None,
                   tok_entropy=None):
    """One stage-2 sample-and-grammar step of `slots` batch rows working through a queue of n_jobs jobs (include/emo_hip.h,
    EMO_GRAMMAR_ACC_QUEUE): logits fp32 [slots, V], tok_out / seg_out int64 [slots], slot_job int32 [slots] (-1: free), mem_lens int64 [slots]
    (the positions the model step reads), row_reset int32 [slots], queue_head int32 [1]; u_steps fp32 [n_u, n_jobs], params / state int32
    [n_jobs, 8], seq / segs int64 [n_jobs, W] and the optional tables (job_steps int32 [n_jobs]; the score tables [n_jobs, W]) are the jobs'.
    Everything but logits, u_steps, params, the lead sheets and the event tables is updated in place."""
    slots, V = logits.shape
    n_jobs = params.shape[0]
    _grammar_once(GRAMMAR_ACC_QUEUE, n_rows=slots, n_token=V, ld_u=n_jobs, n_jobs=n_jobs, mem_rows=mem_rows, temperature=temperature, top_p=top_p,
                  max_len=max_len, track_full=track_full, pad=pad, logits=logits, u_steps=u_steps, ev_flags=ev_flags, ev_beat=ev_beat,
                  lead_tok=lead_tok, lead_off=lead_off, params=params, state=state, seq=seq, segs=segs, tok_out=tok_out, seg_out=seg_out,
                  running=running, slot_job=slot_job, queue_head=queue_head, mem_lens=mem_lens, row_reset=row_reset, job_steps=job_steps,
                  tok_logp=tok_logp, tok_rank=tok_rank, tok_entropy=tok_entropy)
    return tok_out


def acc_window_step(logits, temperature, top_p, u_steps, rows, ev_flags, ev_beat, lead_tok, lead_off, params, state, seq, segs, window, track_full,
                    win_tok, win_seg, running, tok_logp=None, tok_rank=None, tok_entropy=None):
    """One stage-2 draw-and-grammar step of m streams past the window (include/emo_hip.h, EMO_GRAMMAR_ACC_WINDOW): logits fp32 [m, V], win_tok /
    win_seg int64 [m, window]; rows int32 [m] (or None: row b is stream b) names each row's stream in u_steps fp32 [n_u, n], params / state
    int32 [n, 8] and seq / segs int64 [n, width].  state, seq, segs, win_tok, win_seg and running are updated in place.  tok_logp / tok_rank /
    tok_entropy [n, width]: as in txl_grammar_step, indexed by the stream like seq."""
    m, V = logits.shape
    n = state.shape[0]
    assert rows is not None or m <= n
    _grammar_once(GRAMMAR_ACC_WINDOW, n_rows=m, n_token=V, ld_u=n, temperature=temperature, top_p=top_p, window=window, track_full=track_full,
                  logits=logits, u_steps=u_steps, rows=rows, ev_flags=ev_flags, ev_beat=ev_beat, lead_tok=lead_tok, lead_off=lead_off, params=params,
                  state=state, seq=seq, segs=segs, win_tok=win_tok, win_seg=win_seg, running=running, tok_logp=tok_logp, tok_rank=tok_rank,
                  tok_entropy=tok_entropy)
    return win_tok


def acc_rebase(seq, segs, state, params, primer_len, track_leadsheet, keep, W, longest_bar, pad, dst_seq, dst_segs, arch_tok, arch_len, new_len, running,
               scores=None, dst_scores=None, arch_scores=None):
    """Re-anchor the WINDOW rows on a bar (include/emo_hip.h: emo_acc_rebase): seq / segs int64 [n, width] -> dst_seq / dst_segs int64 [n, width2]
    (other buffers), state / params int32 [n, 8] updated in place, primer_len int32 [n], arch_tok int64 [n, cap] with its cursors arch_len int32
    [n], new_len int32 [n], running int32 [1] (+= 1 per row that continues).  scores / dst_scores / arch_scores: the three tables of
    draw_score_tables laid out like seq / dst_seq / arch_tok (dicts with its keys), all three or none.  Allocation-free."""
    n, width = seq.shape
    assert _is(seq, _I64) and _is(segs, _I64) and segs.shape == seq.shape
    assert _is(dst_seq, _I64) and _is(dst_segs, _I64) and dst_seq.shape[0] == n and dst_segs.shape == dst_seq.shape
    assert _is(state, _I32) and state.shape == (n, ACC_STATE_WORDS) and _is(params, _I32) and params.shape == (n, ACC_PARAM_WORDS)
    assert _is(primer_len, _I32) and primer_len.numel() == n and _is(arch_len, _I32) and arch_len.numel() == n
    assert _is(arch_tok, _I64) and arch_tok.dim() == 2 and arch_tok.shape[0] == n
    assert _is(new_len, _I32) and new_len.numel() == n and _is(running, _I32) and running.numel() >= 1
    a = _lib.AccRebase(n_rows=n, seq=ptr(seq), segs=ptr(segs), ld_seq=width, state=ptr(state), params=ptr(params), primer_len=ptr(primer_len),
                       track_leadsheet=int(track_leadsheet), keep=int(keep), window=int(W), longest_bar=int(longest_bar), pad=int(pad),
                       dst_seq=ptr(dst_seq), dst_segs=ptr(dst_segs), ld_dst=dst_seq.shape[1], arch_tok=ptr(arch_tok), arch_len=ptr(arch_len),
                       ld_arch=arch_tok.shape[1], new_len=ptr(new_len), running=ptr(running))
    for t, like, pre in ((scores, seq, 'tok_'), (dst_scores, dst_seq, 'dst_'), (arch_scores, arch_tok, 'arch_')):
        assert (t is None) == (scores is None), 'acc_rebase: the score tables come as sources, destinations and archives, or not at all'
        for key, dt in (('logp', _F32), ('rank', _I32), ('entropy', _F32)):
            if t is not None:
                assert _is(t['tok_' + key], dt) and t['tok_' + key].shape == like.shape
                setattr(a, pre + key, ptr(t['tok_' + key]))
    check(lib.emo_acc_rebase(ctypes.byref(a), stream()))     # (the block lives for this call: the library reads it at call time)
    return new_len


def accuracy_counts(logits, tgt, chord, melody, pad):
    M, V = logits.shape
    counts = torch.zeros(6, device=logits.device, dtype=torch.int64)
    assert logits.is_contiguous() and logits.dtype == torch.float32
    tgt, chord, melody = _c(tgt), _c(chord), _c(melody)
    check(lib.emo_accuracy_counts(ptr(logits), ptr(tgt), ptr(chord), ptr(melody), M, V, pad, ptr(counts), stream()))
    return counts


SUMSQ_FLOATS = 1026     # emo_hip.h: EMO_SUMSQ_FLOATS


def sumsq(x, acc):
    """acc[0] = sum(x*x) in a fixed summation order; acc: SUMSQ_FLOATS fp32 scratch, zeroed once by the caller."""
    assert acc.dtype == torch.float32 and acc.numel() >= SUMSQ_FLOATS
    check(lib.emo_sumsq(ptr(x), x.numel(), ptr(acc), stream()))


def clip_coef(sumsq_t, max_norm, pre, coef, denom=None):
    """coef = pre' * min(1, max_norm / (|g| pre' + 1e-6)), pre' = pre / denom[0] (denom: optional fp32 device scalar)."""
    assert denom is None or (denom.dtype == torch.float32 and denom.numel() >= 1)
    check(lib.emo_clip_coef(ptr(sumsq_t), max_norm, pre, ptr(denom), ptr(coef), stream()))


def adam_step(p, g, m, v, p_bf16, lr, beta1, beta2, eps, step, gscale):
    check(lib.emo_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(p_bf16), p.numel(), lr, beta1, beta2, eps, step, ptr(gscale), stream()))


def transpose_batch(desc, n, total_tiles):
    """desc: device int64 [n, 6] = {src ptr, dst ptr, rows, cols, first tile, tiles per row} (include/emo_hip.h); one launch."""
    check(lib.emo_transpose_batch(ptr(desc), n, total_tiles, stream()))


def add_bias2(x, b1, b2):
    """(x + b1, x + b2): x [M, D] (row-strided view allowed), fp32 biases of D elements (any shape); contiguous outputs in x's dtype, one launch."""
    M, D = x.shape
    assert b1.dtype == torch.float32 and b2.dtype == torch.float32 and b1.numel() == D and b2.numel() == D and b1.is_contiguous() and b2.is_contiguous()
    o1, o2 = torch.empty(M, D, device=x.device, dtype=x.dtype), torch.empty(M, D, device=x.device, dtype=x.dtype)
    check(lib.emo_add_bias2(ptr(x), _rows(x), ptr(b1), ptr(b2), ptr(o1), ptr(o2), dtype_code(x.dtype), M, D, stream()))
    return o1, o2


def cast(src, dst):
    assert src.numel() == dst.numel() and src.is_contiguous() and dst.is_contiguous()
    check(lib.emo_cast(ptr(src), dtype_code(src.dtype), ptr(dst), dtype_code(dst.dtype), src.numel(), stream()))
    return dst
