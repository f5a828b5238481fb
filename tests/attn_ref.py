"""Causal softmax attention (EMO_ATTN_SOFTMAX) and Transformer-XL relative-position attention (EMO_ATTN_RELPOS) as plain references outside the
library: torch on the CPU, float64 unless the caller hands in another dtype; nothing is imported from the package.  Written from
include/emo_hip.h and the header comments of csrc/emo_softmax_attn.hip:

    softmax:  s_ij = q_i.k_j / sqrt(dh) (j <= i),  p = softmax_j(s),  lse_i = log sum_j exp(s_ij),  out_i = sum_j m_ij p_ij v_j
    relpos:   s_ij = ((q_i + u).k_j + (q_i + vb).R[i - j]) / sqrt(dh)  (j <= i; with a window W > 0 also j >= i - W),  p = softmax_j(s),
              zden_i = sum_j m_ij p_ij + 1e-8,  out_i = sum_j m_ij p_ij v_j / zden_i          (softmax -> dropout -> p / (sum p + 1e-8))

m = the dropout multipliers (keep / (1 - p_drop), 1 without a mask), R indexed BY DISTANCE.  Tensors: q, k, v, out [B, T, H, dh]; lse, zden
[B, H, T]; mask [B, H, T, T]; R [n_dist, H, dh]; u, vb [H, dh].  Gradients come from autograd on these functions.

SELECTOR INPUTS make every probability exactly 0 or 1 in fp32, so that an output row of the kernels must EQUAL one row of v:
    softmax:  k_j = the +-1 code of the bits of j (first ceil(log2 T) components, +1 in the rest), q_i = G code(pi(i)) with pi(i) <= i:
              s_ij = G (dh - 2 hamming(pi(i), j)) / sqrt(dh), unique maximum at j = pi(i), gap >= 2 G / sqrt(dh) >= 256 for dh <= 64
    relpos:   q = k = 0, vb[h] = e_0, R[d*_h][h, 0] = G, 0 elsewhere: s_ij = G / sqrt(dh) at i - j = d*_h and 0 elsewhere; rows i < d*_h (or with
              the key i - d*_h outside the window) have uniform probabilities
v holds small integers (distinct rows), so every sum of the backward that meets it is exact too.  tests/test_attn_ref_host.py proves the
one-hot property for every case tests/test_gpu_attn_train_edges.py runs."""
import math

import numpy as np
import torch

G = 1024.0                                 # the selectors' score scale
F64 = torch.float64


def _bh(x):
    """[B, T, H, d] <-> [B, H, T, d]"""
    return x.permute(0, 2, 1, 3)


def _dead(T, window=0):
    """[T, T] bool: key j is not seen by query i"""
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    dead = j > i
    if window > 0:
        dead = dead | (j < i - window)
    return dead


# ------------------------------------------------------------------------------------------- softmax
def softmax_probs(q, k, mask=None):
    """-> (m p [B, H, T, T], lse [B, H, T])"""
    T, dh = q.shape[1], q.shape[3]
    s = (_bh(q) @ _bh(k).transpose(-1, -2)) / math.sqrt(dh)
    s = s.masked_fill(_dead(T), -float('inf'))
    p = torch.softmax(s, -1)
    return (p if mask is None else p * mask), torch.logsumexp(s, -1)


def softmax_ref(q, k, v, mask=None):
    """-> out [B, T, H, dh], lse [B, H, T]"""
    p, lse = softmax_probs(q, k, mask)
    return _bh(p @ _bh(v)), lse


# ------------------------------------------------------------------------------------------- relative position
def relpos_scores(q, k, R, u, vb, window=0):
    """-> s [B, H, T, T] with -inf at the keys a query does not see"""
    T, dh = q.shape[1], q.shape[3]
    ac = torch.einsum('bihd,bjhd->bhij', q + u, k)
    by_dist = torch.einsum('bihd,nhd->bhin', q + vb, R[:T])                              # (q_i + vb).R[n] for every distance n
    dist = (torch.arange(T)[:, None] - torch.arange(T)[None, :]).clamp(min=0)              # i - j (unseen keys: any valid row)
    bd = by_dist.gather(-1, dist.expand(by_dist.shape[0], by_dist.shape[1], T, T))
    return ((ac + bd) / math.sqrt(dh)).masked_fill(_dead(T, window), -float('inf'))


def relpos_probs(q, k, R, u, vb, mask=None, window=0):
    """-> (the final weights m p / zden [B, H, T, T], lse, zden [B, H, T])"""
    s = relpos_scores(q, k, R, u, vb, window)
    p = torch.softmax(s, -1)
    if mask is not None:
        p = p * mask
    zden = p.sum(-1) + 1e-8
    return p / zden[..., None], torch.logsumexp(s, -1), zden


def relpos_ref(q, k, v, R, u, vb, mask=None, window=0):
    """-> out [B, T, H, dh], lse, zden [B, H, T]"""
    a, lse, zden = relpos_probs(q, k, R, u, vb, mask, window)
    return _bh(a @ _bh(v)), lse, zden


# ------------------------------------------------------------------------------------------- selector inputs
def selector_maps(T):
    """name -> pi [T] (long), pi(i) <= i: the maps of the softmax selector"""
    i = torch.arange(T)
    g = torch.Generator().manual_seed(1000 + T)
    return {'diag': i.clone(), 'zero': torch.zeros(T, dtype=torch.long), 'tile0': i - i % 64, 'prev64': (i - 64).clamp(min=0),
            'prev65': (i - 65).clamp(min=0), 'rand': (torch.rand(T, generator=g, dtype=F64) * (i + 1).double()).long().clamp(max=i)}


def _code(idx, nbits, dh):
    """idx [...] long -> [..., dh] of +-1: component c < nbits is +1 where bit c of idx is set, every other component +1"""
    c = torch.ones(idx.shape + (dh,), dtype=F64)
    for b in range(nbits):
        c[..., b] = ((idx >> b) & 1).double() * 2 - 1
    return c


def _int_rows(B, T, H, dh, seed):
    """[B, T, H, dh] of integers in [-127, 127] (exact in bf16), sequence b scaled by (1 + b); no two rows of one (b, h) are equal"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-127, 128, (B, T, H, dh), generator=g).double()
    return v * (1 + torch.arange(B, dtype=F64))[:, None, None, None]


def small_int_dout(B, T, H, dh, seed):
    """[B, T, H, dh] of integers in [-3, 3]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (B, T, H, dh), generator=g).double()


def softmax_selector(B, T, H, dh, pis, seed=0):
    """pis: one map pi [T] per head -> q, k, v [B, T, H, dh] double (every value exact in bf16).  Sequences differ by v alone (scaled by 1 + b):
    the scores must stay at the magnitude G dh / sqrt(dh) for which tests/test_attn_ref_host.py proves the backward's probabilities exact."""
    assert len(pis) == H
    nbits = max(1, int(math.ceil(math.log2(T)))) if T > 1 else 1
    assert nbits <= dh
    k = _code(torch.arange(T), nbits, dh)[None, :, None, :].expand(B, T, H, dh).clone()
    q = torch.stack([G * _code(pi, nbits, dh) for pi in pis], 1)[None].expand(B, T, H, dh).clone()
    return q, k, _int_rows(B, T, H, dh, seed)


def softmax_selector_dv(dout, pis):
    """dv[b, j, h] = sum of dout[b, i, h] over pi_h(i) = j"""
    dv = torch.zeros_like(dout)
    for h, pi in enumerate(pis):
        dv[:, :, h].index_add_(1, pi, dout[:, :, h])
    return dv


def relpos_selector(B, T, H, dh, dstar, seed=0):
    """dstar: one distance per head -> q, k, v [B, T, H, dh], R [T, H, dh], u, vb [H, dh] double"""
    assert len(dstar) == H and all(0 <= d < T for d in dstar)
    g = torch.Generator().manual_seed(seed + 7)
    q, k = torch.zeros(B, T, H, dh, dtype=F64), torch.zeros(B, T, H, dh, dtype=F64)
    R, vb = torch.zeros(T, H, dh, dtype=F64), torch.zeros(H, dh, dtype=F64)
    vb[:, 0] = 1.0
    for h, d in enumerate(dstar):
        R[d, h, 0] = G
    u = torch.randn(H, dh, generator=g, dtype=F64).float().double() * 0.3
    return q, k, _int_rows(B, T, H, dh, seed), R, u, vb


def relpos_selected(T, dstar, window=0):
    """[H, T] long: the key row i of head h selects (i - d*_h), or -1 where the row is uniform (i < d*_h, or the key lies outside the window)"""
    i = torch.arange(T)
    sel = torch.full((len(dstar), T), -1, dtype=torch.long)
    for h, d in enumerate(dstar):
        ok = (i >= d) if window <= 0 else ((i >= d) & (d <= window))
        sel[h, ok] = (i - d)[ok]
    return sel


def one_hot_f32(p, sel):
    """p [B, H, T, T] double, sel [H, T] (-1: row not checked): True when every checked row, rounded to fp32, is exactly the one-hot row of sel"""
    p32 = p.float()
    for h in range(sel.shape[0]):
        rows = torch.nonzero(sel[h] >= 0)[:, 0]
        want = torch.zeros(len(rows), p.shape[-1])
        want[torch.arange(len(rows)), sel[h, rows]] = 1.0
        if not torch.equal(p32[:, h, rows], want[None].expand(p.shape[0], -1, -1)):
            return False
    return True


# ------------------------------------------------------------------------------------------- the bf16 backward's probability at a selected key
def bf16_backward_probability(score, dh, fused32):
    """The probability the bf16 backward kernels recompute at a selected key whose raw score (q.k, before the scale) is `score`, evaluated in
    float32 as the kernels do (csrc/emo_softmax_attn.hip: lse = (s c2) ln2 + log(1), p = exp2(s c2 - lse log2e), c2 = (1 / sqrt(dh)) log2e;
    fused32: csrc/emo_softmax_attn32.hip, lse = ((s c2) ln2), p = exp2(fma(s, c2, -lse log2e))).  The forward's l is exactly 1 for a selector
    row.  -> p as float32 BEFORE its rounding to the bf16 MFMA operand: the dv assertion needs bf16(p) == 1."""
    f = np.float32
    log2e, ln2 = f(1.4426950408889634), f(0.6931471805599453)
    s = f(score)
    if fused32:
        c2 = f(f(1.0) / f(np.sqrt(f(64.0)))) * log2e
        lse = f(f(s * c2) * ln2) + f(0.0)
        e = f(np.float64(s) * np.float64(c2) - np.float64(f(lse * log2e)))              # one rounding: the fma
    else:
        c2 = f(f(1.0) / f(np.sqrt(f(dh)))) * log2e
        lse = f(f(s * c2) * ln2) + f(0.0)
        e = f(f(s * c2) - f(lse * log2e))
    return f(np.exp2(np.float64(e)))


# ------------------------------------------------------------------------------------------- the selector cases (shared by the host proof and the GPU file)
SEL_MAPS = (('diag', 'zero', 'tile0'), ('prev64', 'prev65', 'rand'))          # one map per head, H = 3
SEL_GENERIC = ((65, 64), (129, 64), (193, 64), (129, 16), (129, 32))          # (T, dh) on the generic kernels
SEL_FUSED32 = ((128, 64), (256, 64))                                          # (T, dh) on the 32 x 32 kernels
SEL_RELPOS_T = (193, 130)
SEL_RELPOS_DH = 64


def relpos_dstar(T):
    """The distance triples: the skew buffer's ends, both sides of a key-tile step, the last distance the table holds"""
    return ((0, 1, 15), (16, 63, 64), (65, 79, 80), (127, 128, T - 1))


def relpos_windows(dstar):
    """window 0 (causal), then d* and d* - 1 for every distance of the triple (the selected key inside the band, or just outside it)"""
    return [0] + sorted({w for d in dstar for w in (d, d - 1) if w >= 1})
