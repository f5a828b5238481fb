"""The DECODE pass of emo_attn (GPU): the one-token kernels of the three attention kinds against a plain float64 reference of the same step, at
the lengths, windows and (d_head, n_feat) pairs where their loops change shape.  The caches are longer than their valid prefix and every row
the step must not read is NaN: one row too far, or one row outside the window, ends in a NaN output instead of a plausible number.
Tolerances: the bounds of tests/test_gpu_kernels.py (2e-5 fp32, 3e-2 bf16 of the reference's max-abs) at mult = 3, as its decode comparisons."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DT = [torch.float32, torch.bfloat16]
H3 = 3                                   # heads: blockIdx / H and % H cannot hide behind a power of two
NAN = float('nan')


def _ops():
    from emo_disentanger_amd import ops
    return ops


def _tol(dt):                            # the per-dtype bound of tests/test_gpu_kernels.py
    return 2e-5 if dt == torch.float32 else 3e-2


def _close(got, ref, dt, what, mult=3.0):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert torch.isfinite(got).all(), '%s: not finite' % what
    s = max(float(ref.abs().max()), 1e-6)
    err = float((got - ref).abs().max())
    print('[attn_decode] %s: err/scale %.3e (bound %.1e)' % (what, err / s, mult * _tol(dt)))
    assert err <= mult * _tol(dt) * s, '%s: max err %.3e vs scale %.3e (tol %.1e)' % (what, err, s, mult * _tol(dt))


def _r(*shape, seed=0, dt=torch.float32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dt)


def _bits(t):
    """Integer view: NaN rows compare by their bit pattern."""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _uniq(vals):
    out = []
    for x in vals:
        if x >= 1 and x not in out:
            out.append(x)
    return out


# ------------------------------------------------------------------------------------------- float64 references (one (stream, head) at a time)
def _softmax_ref(q, K, V, lens, H):
    """q [n, H*dh], K / V [n, T_max, H, dh] (row len-1 = the new token), all double: softmax(q.K[:len]^T / sqrt(dh)).V[:len]."""
    n, HD = q.shape
    dh = HD // H
    out = torch.zeros(n, HD, dtype=torch.float64)
    for s in range(n):
        L = int(lens[s])
        for h in range(H):
            sc = (K[s, :L, h] @ q[s, h * dh:(h + 1) * dh]) / math.sqrt(dh)
            out[s, h * dh:(h + 1) * dh] = torch.softmax(sc, 0) @ V[s, :L, h]
    return out


def _relpos_j0(L, mem_len):
    return max(0, L - 1 - mem_len) if mem_len > 0 else 0


def _relpos_ref(q, K, V, lens, H, R, u, vb, mem_len):
    """As _softmax_ref over the keys j0 .. len-1 with score ((q+u).k_j + (q+vb).R[len-1-j]) / sqrt(dh); R [n_dist, H, dh] by distance, u / vb [H, dh].
    The conventions of _relattn_ref in test_gpu_kernels.py (eval: prob = p / (sum p + 1e-8))."""
    n, HD = q.shape
    dh = HD // H
    out = torch.zeros(n, HD, dtype=torch.float64)
    for s in range(n):
        L = int(lens[s])
        j0 = _relpos_j0(L, mem_len)
        for h in range(H):
            qh = q[s, h * dh:(h + 1) * dh]
            dist = [L - 1 - j for j in range(j0, L)]
            sc = (K[s, j0:L, h] @ (qh + u[h]) + R[dist, h] @ (qh + vb[h])) / math.sqrt(dh)
            p = torch.softmax(sc, 0)
            p = p / (p.sum() + 1e-8)
            out[s, h * dh:(h + 1) * dh] = p @ V[s, j0:L, h]
    return out


def _favor_ref_step(q, k, v, om, S, z, H, eps):
    """One recurrent FAVOR+ step in double: z += phi(k), S += phi(k) v^T (in place: S [n, H, F, dh], z [n, H, F]), then out = phi(q).S / (phi(q).z + eps)."""
    from oracle.model_ref import favor_features
    n, HD = q.shape
    dh = HD // H
    out = torch.zeros(n, HD, dtype=torch.float64)
    for s in range(n):
        for h in range(H):
            c = slice(h * dh, (h + 1) * dh)
            pq, pk = favor_features(q[s, c], om), favor_features(k[s, c], om)
            z[s, h] += pk
            S[s, h] += torch.outer(pk, v[s, c])
            out[s, c] = (pq @ S[s, h]) / (pq @ z[s, h] + eps)
    return out


# ------------------------------------------------------------------------------------------- caches: a valid prefix, everything else NaN
def _poisoned(full, lens, lo=None, prefill=False):
    """full [n, T_max, H, dh] (row len-1 = the new token) -> a copy with the rows >= len-1 (prefill: >= len) and, with lo, the rows < lo[s] NaN."""
    c = full.clone()
    for s, L in enumerate(lens):
        c[s, (L if prefill else L - 1):] = NAN
        if lo is not None:
            c[s, :lo[s]] = NAN
    return c


def _device_cache(c, head_major):
    n, T_max, H, dh = c.shape
    return (c.permute(0, 2, 1, 3).contiguous() if head_major else c.reshape(n, T_max, H * dh)).cuda()


def _rows_view(dev, head_major, H):
    """The device cache back as [n, T_max, H, dh] on the host."""
    c = dev.cpu()
    return c.permute(0, 2, 1, 3) if head_major else c.view(c.shape[0], c.shape[1], H, -1)


def _check_appended(dev, before, new, lens, head_major, H, what):
    """before: the host cache [n, T_max, H, dh] as uploaded; new [n, H*dh]: row len-1 holds exactly the new token's row, every other row its old bits."""
    after = _rows_view(dev, head_major, H)
    for s, L in enumerate(lens):
        assert torch.equal(_bits(after[s, L - 1].reshape(-1)), _bits(new[s].cpu())), '%s: stream %d, appended row' % (what, s)
        assert torch.equal(_bits(after[s, :L - 1]), _bits(before[s, :L - 1])), '%s: stream %d, rows below len-1 changed' % (what, s)
        assert torch.equal(_bits(after[s, L:]), _bits(before[s, L:])), '%s: stream %d, rows from len on changed' % (what, s)


# ------------------------------------------------------------------------------------------- softmax decode
def _sattn_geometry(dt, dh, nt):
    """sattn_decode_kernel (emo_softmax_attn.hip): VE = 16 / sizeof(CT), LPR = dh / VE lanes per key row, RPB = NT / LPR rows per block pass,
    SU = NT >= 1024 ? 4 : 8 rows per thread in flight; one sweep of the score / value loops covers RPB * SU keys."""
    ve = 8 if dt == torch.bfloat16 else 4
    rpb = nt // (dh // ve)
    return rpb, rpb * (4 if nt >= 1024 else 8)


def _sattn_env(monkeypatch, nt):
    if nt == 256:
        monkeypatch.setenv('EMO_SATTN_DECODE_NT', '256')
    else:
        monkeypatch.delenv('EMO_SATTN_DECODE_NT', raising=False)


@pytest.mark.parametrize('nt', [1024, 256])
@pytest.mark.parametrize('head_major', [False, True])
@pytest.mark.parametrize('dh', [16, 32, 64, 128])
@pytest.mark.parametrize('dt', DT)
def test_softmax_decode_ragged_lengths_vs_float64(dt, dh, head_major, nt, monkeypatch):
    """One launch, one stream per length 1, 2, RPB-1, RPB, RPB+1, sweep-1, sweep, sweep+1, T_max = 2 sweep + 3: either side of a row-block pass and
    of a key sweep (the clamped tail loads), and a full cache."""
    ops = _ops()
    _sattn_env(monkeypatch, nt)
    H = H3
    HD = H * dh
    rpb, sweep = _sattn_geometry(dt, dh, nt)
    T_max = 2 * sweep + 3
    lens = _uniq([1, 2, rpb - 1, rpb, rpb + 1, sweep - 1, sweep, sweep + 1, T_max])
    n = len(lens)
    qkv = _r(n, 3 * HD, seed=21, dt=dt)
    K, V = _r(n, T_max, H, dh, seed=22, dt=dt), _r(n, T_max, H, dh, seed=23, dt=dt)
    for s, L in enumerate(lens):
        K[s, L - 1] = qkv[s, HD:2 * HD].view(H, dh)
        V[s, L - 1] = qkv[s, 2 * HD:].view(H, dh)
    ref = _softmax_ref(qkv[:, :HD].double(), K.double(), V.double(), lens, H)
    qc = qkv.cuda()
    q, k_new, v_new = qc[:, :HD], qc[:, HD:2 * HD], qc[:, 2 * HD:]            # column slices: the row stride is not the width
    lens_d = torch.tensor(lens, dtype=torch.int64, device='cuda')
    tag = 'softmax %s dh%d %s nt%d' % ('bf16' if dt == torch.bfloat16 else 'fp32', dh, 'head-major' if head_major else 'row-major', nt)

    kp, vp = _poisoned(K, lens), _poisoned(V, lens)                           # NaN from row len-1 on, the row to append included
    kc, vc = _device_cache(kp, head_major), _device_cache(vp, head_major)
    out = ops.softmax_attn_decode(q, kc, vc, lens_d, H, k_new=k_new, v_new=v_new)
    _close(out, ref, dt, tag)
    _check_appended(kc, kp, k_new, lens, head_major, H, tag + ' K')
    _check_appended(vc, vp, v_new, lens, head_major, H, tag + ' V')

    kc1, vc1 = _device_cache(kp, head_major), _device_cache(vp, head_major)   # the same step as lens - 1 with lens_off = 1
    out1 = ops.softmax_attn_decode(q, kc1, vc1, lens_d - 1, H, lens_off=1, k_new=k_new, v_new=v_new)
    assert torch.equal(_bits(out1), _bits(out)), tag + ': lens_off = 1 differs from lens_off = 0'
    assert torch.equal(_bits(kc1), _bits(kc)) and torch.equal(_bits(vc1), _bits(vc))

    kf, vf = _poisoned(K, lens, prefill=True), _poisoned(V, lens, prefill=True)     # nothing to append: row len-1 is already there
    kc2, vc2 = _device_cache(kf, head_major), _device_cache(vf, head_major)
    k0, v0 = kc2.clone(), vc2.clone()
    out2 = ops.softmax_attn_decode(q, kc2, vc2, lens_d, H)
    _close(out2, ref, dt, tag + ' no new rows')
    assert torch.equal(_bits(kc2), _bits(k0)) and torch.equal(_bits(vc2), _bits(v0)), tag + ': a call without k / v wrote to the caches'


@pytest.mark.parametrize('T_max', [24577, 32768])
@pytest.mark.parametrize('dt', DT)
def test_softmax_decode_full_score_buffer_vs_float64(dt, T_max):
    """One stream, one head of d_head 16 with lens = T_max: 24577 keys = the first score buffer over 96 KiB, where the launcher itself takes the
    256-thread instance; 32768 = the largest the entry admits (128 KiB of scores)."""
    ops = _ops()
    H, dh = 1, 16
    qkv = _r(1, 3 * dh, seed=31, dt=dt)
    K, V = _r(1, T_max, H, dh, seed=32, dt=dt), _r(1, T_max, H, dh, seed=33, dt=dt)
    K[0, T_max - 1], V[0, T_max - 1] = qkv[0, dh:2 * dh].view(H, dh), qkv[0, 2 * dh:].view(H, dh)
    ref = _softmax_ref(qkv[:, :dh].double(), K.double(), V.double(), [T_max], H)
    qc = qkv.cuda()
    kp, vp = _poisoned(K, [T_max]), _poisoned(V, [T_max])
    kc, vc = _device_cache(kp, False), _device_cache(vp, False)
    out = ops.softmax_attn_decode(qc[:, :dh], kc, vc, torch.tensor([T_max], dtype=torch.int64, device='cuda'), H, k_new=qc[:, dh:2 * dh], v_new=qc[:, 2 * dh:])
    tag = 'softmax %s T_max %d' % ('bf16' if dt == torch.bfloat16 else 'fp32', T_max)
    _close(out, ref, dt, tag)
    _check_appended(kc, kp, qc[:, dh:2 * dh], [T_max], False, H, tag + ' K')
    _check_appended(vc, vp, qc[:, 2 * dh:], [T_max], False, H, tag + ' V')


# ------------------------------------------------------------------------------------------- relative-position decode
@pytest.mark.parametrize('dh', [16, 32, 64, 128])
@pytest.mark.parametrize('dt', DT)
def test_relpos_decode_ragged_lengths_and_windows_vs_float64(dt, dh):
    """relattn_decode_kernel (emo_softmax_attn.hip): VE = 16 / sizeof(CT), LPR = dh / VE, RPB = 256 / LPR key rows per block pass (no SU).  One stream
    per length 1, 2, RPB-1, RPB, RPB+1, 2 RPB + 1 of T_max = 2 RPB + 3, for every mem_len that puts j0 = len-1-mem_len at 0, the window on either
    side of a row block, or past the whole cache.  NaN in the cache rows < j0 and >= len-1 and in every r_dist row (and pad column) past the largest
    distance of the launch."""
    ops = _ops()
    H = H3
    HD = H * dh
    ve = 8 if dt == torch.bfloat16 else 4
    rpb = 256 // (dh // ve)
    T_max = 2 * rpb + 3
    lens = _uniq([1, 2, rpb - 1, rpb, rpb + 1, 2 * rpb + 1])
    n = len(lens)
    qkv = _r(n, 3 * HD, seed=41, dt=dt, scale=0.7)
    K, V = _r(n, T_max, H, dh, seed=42, dt=dt, scale=0.7), _r(n, T_max, H, dh, seed=43, dt=dt)
    for s, L in enumerate(lens):
        K[s, L - 1] = qkv[s, HD:2 * HD].view(H, dh)
        V[s, L - 1] = qkv[s, 2 * HD:].view(H, dh)
    R = _r(T_max, HD, seed=44, dt=dt, scale=0.7)
    u, vb = _r(H, dh, seed=45, scale=0.3), _r(H, dh, seed=46, scale=0.3)
    qc, uc, vbc = qkv.cuda(), u.cuda(), vb.cuda()
    q, k_new, v_new = qc[:, :HD], qc[:, HD:2 * HD], qc[:, 2 * HD:]
    lens_d = torch.tensor(lens, dtype=torch.int64, device='cuda')
    for mem_len in sorted({0, 1, rpb - 1, rpb, rpb + 1, T_max - 2, T_max - 1, T_max + 5}):
        tag = 'relpos %s dh%d mem_len %d' % ('bf16' if dt == torch.bfloat16 else 'fp32', dh, mem_len)
        ref = _relpos_ref(qkv[:, :HD].double(), K.double(), V.double(), lens, H, R.double().view(T_max, H, dh), u.double(), vb.double(), mem_len)
        lo = [_relpos_j0(L, mem_len) for L in lens]
        far = max(L - 1 - j for L, j in zip(lens, lo))                        # the largest distance any stream of the launch reads
        Rp = R.clone()
        Rp[far + 1:] = NAN
        wide = torch.full((T_max + 5, HD + 2 * ve), NAN, dtype=dt)            # more rows, a wider row stride, 16-B aligned column slice
        wide[:far + 1, ve:ve + HD] = R[:far + 1]
        kp, vp = _poisoned(K, lens, lo), _poisoned(V, lens, lo)

        kc, vc = _device_cache(kp, False), _device_cache(vp, False)
        out = ops.relpos_attn_decode(q, kc, vc, lens_d, H, Rp.cuda(), uc, vbc, mem_len=mem_len, k_new=k_new, v_new=v_new)
        _close(out, ref, dt, tag)
        _check_appended(kc, kp, k_new, lens, False, H, tag + ' K')
        _check_appended(vc, vp, v_new, lens, False, H, tag + ' V')

        kc1, vc1 = _device_cache(kp, False), _device_cache(vp, False)         # lens - 1 with lens_off = 1, r_dist as a slice of a larger tensor
        out1 = ops.relpos_attn_decode(q, kc1, vc1, lens_d - 1, H, wide.cuda()[:, ve:ve + HD], uc, vbc, mem_len=mem_len, lens_off=1, k_new=k_new, v_new=v_new)
        _close(out1, ref, dt, tag + ' wide r_dist')
        assert torch.equal(_bits(out1), _bits(out)), tag + ': lens_off = 1 / strided r_dist differs'
        assert torch.equal(_bits(kc1), _bits(kc)) and torch.equal(_bits(vc1), _bits(vc))

        kf, vf = _poisoned(K, lens, lo, prefill=True), _poisoned(V, lens, lo, prefill=True)
        kc2, vc2 = _device_cache(kf, False), _device_cache(vf, False)
        k0, v0 = kc2.clone(), vc2.clone()
        out2 = ops.relpos_attn_decode(q, kc2, vc2, lens_d, H, Rp.cuda(), uc, vbc, mem_len=mem_len)
        _close(out2, ref, dt, tag + ' no new rows')
        assert torch.equal(_bits(kc2), _bits(k0)) and torch.equal(_bits(vc2), _bits(v0)), tag + ': a call without k / v wrote to the caches'


# ------------------------------------------------------------------------------------------- FAVOR+ decode
# (d_head, n_feat): the five compile-time instances of favor_decode (emo_favor.hip), then three pairs that only the generic kernel serves
FAVOR_PAIRS = [(64, 128), (32, 128), (32, 64), (16, 32), (16, 64), (64, 64), (16, 128), (64, 32)]


@pytest.mark.parametrize('generic', [False, True])
@pytest.mark.parametrize('dh,nf', FAVOR_PAIRS)
@pytest.mark.parametrize('dt', DT)
def test_favor_decode_steps_and_state_vs_float64(dt, dh, nf, generic, monkeypatch):
    """4 consecutive steps of 5 streams x 3 heads from a non-zero state: after every step the output, state_S and state_z against the float64
    recurrence (which never sees the kernel's state).  The state is fp32 for both dtypes and both sides get the same rounded inputs: fp32 bound."""
    ops = _ops()
    from oracle.weights import orthogonal_omega
    if generic:
        monkeypatch.setenv('EMO_FAVOR_DECODE_GENERIC', '1')
    else:
        monkeypatch.delenv('EMO_FAVOR_DECODE_GENERIC', raising=False)
    n, H, eps = 5, H3, 1e-6
    HD = H * dh
    om = orthogonal_omega(dh, nf, np.random.default_rng(6))
    S0, z0 = _r(n, H, nf, dh, seed=52), _r(n, H, nf, seed=53).abs() + 1.0
    S, z = S0.cuda(), z0.cuda()
    Sr, zr = S0.double(), z0.double()
    omc = om.cuda()
    tag = 'favor %s (%d, %d) %s' % ('bf16' if dt == torch.bfloat16 else 'fp32', dh, nf, 'generic' if generic else 'default')
    for step in range(4):
        qkv = _r(n, 3 * HD, seed=60 + step, dt=dt, scale=0.8)
        ref = _favor_ref_step(qkv[:, :HD].double(), qkv[:, HD:2 * HD].double(), qkv[:, 2 * HD:].double(), om.double(), Sr, zr, H, eps)
        qc = qkv.cuda()
        out = ops.favor_decode_step(qc[:, :HD], qc[:, HD:2 * HD], qc[:, 2 * HD:], omc, S, z, H, eps=eps)
        _close(out, ref, dt, '%s step %d out' % (tag, step))
        _close(S, Sr, torch.float32, '%s step %d state_S' % (tag, step))
        _close(z, zr, torch.float32, '%s step %d state_z' % (tag, step))
