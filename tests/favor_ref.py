"""FAVOR+ causal linear attention, forward and backward, as a plain O(T^2) reference outside the library (torch on the CPU, float64 unless the
caller hands in another dtype; nothing is imported from the package).  Written from include/emo_hip.h (EMO_ATTN_FAVOR) and the header comment of
csrc/emo_favor.hip:

    phi(x)  = [exp(u - off), exp(-u - off)],  u = (c x) omega,  c = dh^-1/4,  off = |c x|^2 / 2 + ln(F) / 2,  F = 2 * omega.shape[1]
    S_t = sum_{j<=t} phi(k_j) (x) v_j,  z_t = sum_{j<=t} phi(k_j),  den_t = phi(q_t).z_t + eps,  out_t = phi(q_t)^T S_t / den_t
    dN_t = dout_t / den_t,  dD_t = -(dout_t.out_t) / den_t,  P_tj = dN_t.v_j + dD_t  (j <= t)
    dPhiq_t = sum_{j<=t} P_tj phi(k_j),  dPhik_j = sum_{t>=j} P_tj phi(q_t),  dv_j = sum_{t>=j} (phi(q_t).phi(k_j)) dN_t
    a = dPhi * phi,  dx_d = c sum_m omega_dm (a+_m - a-_m) - c^2 x_d sum_f a_f          (the feature map's Jacobian; a+ / a- = the two halves)

Tensors: q, k, v, dout, out and the gradients [B, T, H, dh]; den [B, H, T]; S [B, H, F, dh]; z [B, H, F].

Every quantity has a MAGNITUDE COMPANION: the same sums over the absolute values of their terms (features are positive, so for `out` it is the
attention applied to |v|).  The companions are multilinear in (phi(q), phi(k), (|dN|, |dD|)), which is what error bounds need: a relative
error e_q of phi(q) contributes companion(phi(q) e_q, phi(k), ...), an error of dN contributes companion(..., |error of dN|) and so on; see
`Bounds`.  The seeded defects of tests/test_favor_ref_host.py are parameters here (`mask`, `ln_f`, `state_upto`, `no_dd`, `no_suma`, `dd_over_den`)."""
import math

import torch

FLOOR = 2.0 ** -80      # absolute floor of every bound: products under 2^-126 may flush to zero, <= T * F of them per sum, divided by den >= eps


def _bh(x):
    """[B, T, H, d] -> [B, H, T, d]"""
    return x.permute(0, 2, 1, 3)


def arg_sizes(x, omega):
    """A [..., F] = sum_d |c x_d omega_dm| (the same for both halves) and off [..., 1] of the FAVOR+ features: the sizes of the exp's argument"""
    dh = x.shape[-1]
    c = dh ** -0.25
    A = (c * x).abs() @ omega.abs()
    off = 0.5 * ((c * x) ** 2).sum(-1, keepdim=True) + 0.5 * math.log(2 * omega.shape[1])
    return torch.cat([A, A], -1), off


def features(x, omega, ln_f=True):
    """x [..., dh], omega [dh, F/2] -> phi(x) [..., F]"""
    dh = x.shape[-1]
    c = dh ** -0.25
    u = (c * x) @ omega
    off = 0.5 * ((c * x) ** 2).sum(-1, keepdim=True) + (0.5 * math.log(2 * omega.shape[1]) if ln_f else 0.0)
    return torch.cat([torch.exp(u - off), torch.exp(-u - off)], -1)


def causal_mask(T, dtype=torch.float64):
    return torch.tril(torch.ones(T, T, dtype=dtype))            # [t, j]: j <= t


def _fwd_core(FQ, FK, V, M, eps, state_upto=None):
    """FQ, FK [B,H,T,F], V [B,H,T,dh], M [T,T] -> num [B,H,T,dh], den - eps .. the plain sums; V = |v| gives the companions"""
    A = (FQ @ FK.transpose(-1, -2)) * M
    n = FK.shape[2] if state_upto is None else state_upto
    return A, A @ V, A.sum(-1) + eps, FK[:, :, :n].transpose(-1, -2) @ V[:, :, :n], FK[:, :, :n].sum(2)


def forward(q, k, v, omega, eps=1e-6, mask=None, ln_f=True, state_upto=None):
    """-> dict(out [B,T,H,dh], den [B,H,T], S [B,H,F,dh], z [B,H,F])"""
    M = causal_mask(q.shape[1], q.dtype) if mask is None else mask
    FQ, FK = features(_bh(q), omega, ln_f), features(_bh(k), omega, ln_f)
    _, num, den, S, z = _fwd_core(FQ, FK, _bh(v), M, eps, state_upto)
    return dict(out=_bh(num / den[..., None]), den=den, S=S, z=z)


def _bwd_core(FQ, FK, V, GN, GD, W, xq, xk, M, signed, no_suma=False):
    """The gradient sums for (dN, dD) = (GN [B,H,T,dh], GD [B,H,T]); signed=False: every difference becomes a sum (companions: hand in absolute values)"""
    dh, mf = xq.shape[-1], W.shape[1]
    c = dh ** -0.25
    A = (FQ @ FK.transpose(-1, -2)) * M
    P = (GN @ V.transpose(-1, -2) + GD[..., None]) * M                                     # [t, j]

    def jac(a, x):
        diff = (a[..., :mf] - a[..., mf:]) if signed else (a[..., :mf] + a[..., mf:])
        sa = a.sum(-1, keepdim=True) * (0.0 if no_suma else 1.0)
        return c * (diff @ W.transpose(-1, -2)) + (-1.0 if signed else 1.0) * c * c * x * sa
    dq = jac((P @ FK) * FQ, xq)
    dk = jac((P.transpose(-1, -2) @ FQ) * FK, xk)
    dv = A.transpose(-1, -2) @ GN
    return dq, dk, dv


def backward(q, k, v, omega, dout, eps=1e-6, dn=False, mask=None, ln_f=True, no_dd=False, no_suma=False, dd_over_den=False, out=None, den=None):
    """Closed-form backward.  dn=True: `dout` holds dN = dout / den (the dout_is_dn form); den is then not used.  out / den: the forward's
    results when the caller wants the gradients for given ones (default: the reference's own).  -> dict(dq, dk, dv [B,T,H,dh], dN, dD)"""
    M = causal_mask(q.shape[1], q.dtype) if mask is None else mask
    if out is None or (den is None and (not dn or dd_over_den)):
        f = forward(q, k, v, omega, eps, M, ln_f)
        out = f['out'] if out is None else out
        den = f['den'] if den is None else den
    FQ, FK = features(_bh(q), omega, ln_f), features(_bh(k), omega, ln_f)
    g, o = _bh(dout), _bh(out)
    if dn:
        dN, dD = g, -(g * o).sum(-1)
        if dd_over_den:                                           # seeded defect: dD formed as if `dout` were the undivided gradient
            dD = dD / den
    else:
        dN, dD = g / den[..., None], -(g * o).sum(-1) / den
    if no_dd:
        dD = torch.zeros_like(dD)
    dq, dk, dv = _bwd_core(FQ, FK, _bh(v), dN, dD, omega, _bh(q), _bh(k), M, True, no_suma)
    return dict(dq=_bh(dq), dk=_bh(dk), dv=_bh(dv), dN=dN, dD=dD)


class Bounds:
    """|got - ref| <= k u mag + (the argument-size terms) + (what the errors of den and out do to dN, dD) + u_store |ref|, element by element.

    k: dict quantity -> count of roundings (tests/test_gpu_favor_edges.py derives them); u: unit round-off of the path.
    rho(x) [..., F]: relative error of a feature in units of u beyond the counted roundings — the argument-size terms: the returned features
    carry a relative error <= expm1(u rho).  u_store: rounding of out and the gradients; u_g: rounding of dN (0 in the dout_is_dn form, where
    dN is an input); u_dd: rounding of dD."""

    def __init__(self, q, k, v, omega, dout, eps, kk, u, rho, u_store, u_g, u_dd, dn=False):
        T = q.shape[1]
        M = causal_mask(T)
        f = forward(q, k, v, omega, eps)
        xq, xk, V = _bh(q), _bh(k), _bh(v).abs()
        FQ, FK = features(xq, omega), features(xk, omega)
        YQ, YK = FQ * torch.expm1(u * rho(xq)) / u, FK * torch.expm1(u * rho(xk)) / u     # phi * (relative error / u)

        def fwd_err(kn, kd):
            _, n0, d0, S0, z0 = _fwd_core(FQ, FK, V, M, 0.0)
            _, n1, d1, S1, z1 = _fwd_core(YQ, FK, V, M, 0.0)
            _, n2, d2, S2, z2 = _fwd_core(FQ, YK, V, M, 0.0)
            _, n3, d3, _, _ = _fwd_core(YQ, YK, V, M, 0.0)
            return (u * (kn * n0 + n1 + n2 + u * n3), u * (kd * d0 + d1 + d2 + u * d3), u * (kk['S'] * S0 + S2), u * (kk['z'] * z0 + z2), n0)
        e_num, e_den, e_S, e_z, mag_num = fwd_err(kk['num'], kk['den'])
        den, out = f['den'], _bh(f['out'])
        r = e_den / den
        assert float(r.max()) < 0.5, 'the bound of den exceeds half of den: the first-order model does not hold'
        r1 = r / (1 - r)
        e_out = (e_num + out.abs() * e_den[..., None]) / (den * (1 - r))[..., None]
        self.ref = dict(f)
        self.mag = dict(out=_bh(mag_num / den[..., None]), den=den - eps)
        # den, S, z are stored in float32: one rounding of the stored value; den also carries float32(eps) and the rounding of `+ eps`
        u32 = 2.0 ** -24
        self.bound = dict(out=_bh(e_out + u_store * out.abs()) + FLOOR, den=e_den + 2 * u32 * den + FLOOR,
                          S=e_S + u32 * f['S'].abs() + FLOOR, z=e_z + u32 * f['z'].abs() + FLOOR)
        if dout is None:
            return
        b = backward(q, k, v, omega, dout, eps, dn=dn)
        g = _bh(dout).abs()
        e_o = e_out + u_store * out.abs()                          # the backward reads the STORED out
        if dn:
            GN, GD = g, (g * out.abs()).sum(-1)
            eN, eD = torch.zeros_like(GN), (g * e_o).sum(-1) + u_dd * GD
        else:
            GN, GD = g / den[..., None], (g * out.abs()).sum(-1) / den
            eN, eD = GN * (u_g + r1)[..., None], (g * e_o).sum(-1) / den * (1 + r1) + GD * (r1 + u_dd)
        W = omega.abs()
        G1, D1 = GN + eN, GD + eD
        m0 = _bwd_core(FQ, FK, V, G1, D1, W, xq.abs(), xk.abs(), M, False)
        m1 = _bwd_core(YQ, FK, V, G1, D1, W, xq.abs(), xk.abs(), M, False)
        m2 = _bwd_core(FQ, YK, V, G1, D1, W, xq.abs(), xk.abs(), M, False)
        m3 = _bwd_core(YQ, YK, V, G1, D1, W, xq.abs(), xk.abs(), M, False)
        me = _bwd_core(FQ, FK, V, eN, eD, W, xq.abs(), xk.abs(), M, False)
        mg = _bwd_core(FQ, FK, V, GN, GD, W, xq.abs(), xk.abs(), M, False)
        for i, name in enumerate(('dq', 'dk', 'dv')):
            self.ref[name] = b[name]
            self.mag[name] = _bh(mg[i])
            self.bound[name] = _bh(u * (kk[name] * m0[i] + m1[i] + m2[i] + u * m3[i]) + me[i]) + u_store * b[name].abs() + FLOOR

    def ratio(self, name, got):
        """max |got - ref| / bound of one quantity (inf for a non-finite result)"""
        got = got.double()
        if not bool(torch.isfinite(got).all()):
            return float('inf')
        return float(((got - self.ref[name]).abs() / self.bound[name]).max())


def emulate(q, k, v, omega, dout, eps, chunk, lowp, dn=False):
    """The chunked evaluation the kernels perform, in float32: per chunk of `chunk` tokens (one size, or three: forward, dq sweep, dk/dv sweep) a
    masked product inside the chunk plus the carried state.  lowp: omega, the features, the masked chunk matrices, the carried state's operand copy, dN, the Jacobian's operand and the outputs are
    rounded to bf16 (float32 accumulation throughout), as the bf16 kernels do.  Returns the quantities of forward() and backward() (dN given: dn)."""
    f32 = torch.float32
    rb = (lambda t: t.bfloat16().float()) if lowp else (lambda t: t)
    xq, xk, V = [_bh(t).to(f32) for t in (q, k, v)]
    B, H, T, dh = xq.shape
    W = rb(omega.to(f32))
    mf = W.shape[1]
    c = dh ** -0.25
    FQ, FK = rb(features(xq, W)), rb(features(xk, W))
    F = FQ.shape[-1]
    out, den = torch.zeros(B, H, T, dh), torch.zeros(B, H, T)
    S, z = torch.zeros(B, H, F, dh), torch.zeros(B, H, F)
    cf, cq, ck = (chunk, chunk, chunk) if isinstance(chunk, int) else chunk
    for t0 in range(0, T, cf):
        s = slice(t0, min(t0 + cf, T))
        A = rb((FQ[:, :, s] @ FK[:, :, s].transpose(-1, -2)) * causal_mask(s.stop - s.start, f32))
        den[:, :, s] = A.sum(-1) + (FQ[:, :, s] * z[:, :, None, :]).sum(-1) + eps
        out[:, :, s] = rb((A @ V[:, :, s] + FQ[:, :, s] @ rb(S)) / den[:, :, s, None])
        S = S + FK[:, :, s].transpose(-1, -2) @ V[:, :, s]
        z = z + FK[:, :, s].sum(2)
    res = dict(out=_bh(out), den=den, S=S, z=z)
    if dout is None:
        return res
    g = _bh(dout).to(f32)
    if dn:
        G, dD = g, -(g * out).sum(-1)
    else:
        G, dD = rb(g / den[..., None]), -(g * out).sum(-1) / den

    def jac(a, x):
        ad = rb(a[..., :mf] - a[..., mf:])
        return rb(c * (ad @ W.transpose(-1, -2) - c * x * a.sum(-1, keepdim=True)))
    dq, dk, dv = torch.zeros_like(xq), torch.zeros_like(xq), torch.zeros_like(xq)
    S, z = torch.zeros(B, H, F, dh), torch.zeros(B, H, F)
    for t0 in range(0, T, cq):                                    # the dq sweep
        s = slice(t0, min(t0 + cq, T))
        P = rb((G[:, :, s] @ V[:, :, s].transpose(-1, -2) + dD[:, :, s, None]) * causal_mask(s.stop - s.start, f32))
        dphi = P @ FK[:, :, s] + G[:, :, s] @ rb(S).transpose(-1, -2) + dD[:, :, s, None] * z[:, :, None, :]
        dq[:, :, s] = jac(dphi * FQ[:, :, s], xq[:, :, s])
        S = S + FK[:, :, s].transpose(-1, -2) @ V[:, :, s]
        z = z + FK[:, :, s].sum(2)
    R, r = torch.zeros(B, H, F, dh), torch.zeros(B, H, F)
    for t0 in reversed(range(0, T, ck)):                          # the reverse sweep: dk, dv
        s = slice(t0, min(t0 + ck, T))
        Mc = causal_mask(s.stop - s.start, f32)
        P = rb((G[:, :, s] @ V[:, :, s].transpose(-1, -2) + dD[:, :, s, None]) * Mc)
        A = rb((FQ[:, :, s] @ FK[:, :, s].transpose(-1, -2)) * Mc)
        dphi = P.transpose(-1, -2) @ FQ[:, :, s] + V[:, :, s] @ rb(R).transpose(-1, -2) + r[:, :, None, :]
        dk[:, :, s] = jac(dphi * FK[:, :, s], xk[:, :, s])
        dv[:, :, s] = rb(A.transpose(-1, -2) @ G[:, :, s] + FK[:, :, s] @ rb(R))
        R = R + FQ[:, :, s].transpose(-1, -2) @ G[:, :, s]
        r = r + (FQ[:, :, s] * dD[:, :, s, None]).sum(2)
    res.update(dq=_bh(dq), dk=_bh(dk), dv=_bh(dv))
    return res
