#!/usr/bin/env python3
"""Which kernels emo_attn launches, case by case: one labelled call per routing decision of the attention host code (slice / 32 x 32 / generic
instances, segmented scan, decode instances, RELPOS band / causal), each behind a separator launch (favor_omega_kernel) and a synchronise.

  rocprofv3 --kernel-trace -f csv -d DIR -o x -- python tools/attn_routing.py LABELS      # run the cases (kernel trace alone, no counters)
  python tools/attn_routing.py --names DIR/x_kernel_trace.csv LABELS                      # -> JSON {label: [kernel names in launch order]}

Two library builds route alike when the two JSON documents are equal."""
import csv, json, os, re, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEPARATOR = 'favor_omega_kernel'
SWITCHES = ('EMO_FAVOR_FS', 'EMO_FAVOR_FS_BWD', 'EMO_FAVOR_SEGMENTS', 'EMO_SATTN32', 'EMO_SATTN32_BWD', 'EMO_SATTN32_DQ', 'EMO_SATTN_DECODE_NT',
            'EMO_FAVOR_DECODE_GENERIC')


def cases():
    """[(label, {switch: value}, thunk)], in a fixed order.  Inputs are made here, before the first labelled call."""
    import numpy as np
    import torch
    from emo_disentanger_amd import ops
    from emo_disentanger_amd.ops import ATTN_BWD, ATTN_BWD_KV, ATTN_BWD_R, ATTN_RELPOS, _attn, _rows, ptr
    from oracle.weights import orthogonal_omega
    bf, f32 = torch.bfloat16, torch.float32
    rnd = lambda *s, dt=f32: (torch.randn(*s, device='cuda') * 0.7).to(dt)
    B, H, out = 1, 2, []

    def favor(tag, env, T=64, dt=bf, dh=64, nf=128, segs='1'):
        HD = H * dh
        om = orthogonal_omega(dh, nf, np.random.default_rng(6)).cuda()
        qkv, dout = rnd(B * T, 3 * HD, dt=dt), rnd(B * T, HD, dt=dt)
        q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
        env = dict(env, EMO_FAVOR_SEGMENTS=segs)
        o, den = ops.favor_attn_fwd(q, k, v, om, B, T, H)
        out.append(('favor fwd ' + tag, env, lambda: ops.favor_attn_fwd(q, k, v, om, B, T, H)))
        out.append(('favor bwd ' + tag, env, lambda: ops.favor_attn_bwd(q, k, v, om, o, dout, den, B, T, H)))
        return q, k, v, om, o, dout, den, env

    served = favor('slice kernels, T=64', {})
    out.append(('favor bwd dn, T=64', served[-1], lambda a=served[:-1]: ops.favor_attn_bwd(*a, B, 64, H, dn=True)))
    favor('T=48', {}, T=48)
    favor('fp32', {}, dt=f32)
    favor('d_head 32', {}, dh=32)
    favor('EMO_FAVOR_FS=0', {'EMO_FAVOR_FS': '0'})
    favor('EMO_FAVOR_FS_BWD=0', {'EMO_FAVOR_FS_BWD': '0'})
    seg = favor('segmented T=256, kstate_valid 0', {}, T=256, segs='2')
    os.environ['EMO_FAVOR_SEGMENTS'] = '2'
    ws_kept = ops.favor_attn_fwd(*seg[:4], B, 256, H, keep_ws=True)[2]
    del os.environ['EMO_FAVOR_SEGMENTS']
    out.append(('favor bwd segmented T=256, kstate_valid 1', seg[-1], lambda a=seg[:-1], w=ws_kept: ops.favor_attn_bwd(*a, B, 256, H, ws_saved=w)))

    n, dh, nf = 3, 32, 64
    HD = H * dh
    omd = orthogonal_omega(dh, nf, np.random.default_rng(6)).cuda()
    row = rnd(n, 3 * HD, dt=bf)
    qd, kd, vd = row[:, :HD], row[:, HD:2 * HD], row[:, 2 * HD:]
    S, z = rnd(n, H, nf, dh), rnd(n, H, nf).abs() + 1.0
    S8 = rnd(n * H * nf * dh + 4)[2:-2].view(n, H, nf, dh)          # 8-byte but not 16-byte aligned
    assert S8.data_ptr() % 16 == 8
    out.append(('favor decode fast', {}, lambda: ops.favor_decode_step(qd, kd, vd, omd, S, z, H)))
    out.append(('favor decode EMO_FAVOR_DECODE_GENERIC', {'EMO_FAVOR_DECODE_GENERIC': '1'}, lambda: ops.favor_decode_step(qd, kd, vd, omd, S, z, H)))
    out.append(('favor decode state_S 8-B aligned', {}, lambda: ops.favor_decode_step(qd, kd, vd, omd, S8, z, H)))

    def softmax(tag, env, T=128, dt=bf, dh=64, p=0.1, keep=True):
        HD = H * dh
        qkv, dout = rnd(B * T, 3 * HD, dt=dt), rnd(B * T, HD, dt=dt)
        q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
        for name, val in env.items():
            os.environ[name] = val
        res = ops.softmax_attn_fwd(q, k, v, B, T, H, p_drop=p, seed=3, offset=9, want_keep=keep)
        for name in env:
            del os.environ[name]
        o, lse, kw = res if keep else res + (None,)
        out.append(('softmax fwd ' + tag, env, lambda: ops.softmax_attn_fwd(q, k, v, B, T, H, p_drop=p, seed=3, offset=9, want_keep=keep)))
        out.append(('softmax bwd ' + tag, env, lambda: ops.softmax_attn_bwd(q, k, v, o, dout, lse, B, T, H, p_drop=p, seed=3, offset=9, keep=kw)))

    softmax('32 x 32, keep words', {})
    softmax('32 x 32, no keep words', {}, keep=False)
    softmax('32 x 32, p_drop 0', {}, p=0.0)
    softmax('T=192', {}, T=192)
    softmax('d_head 32', {}, dh=32)
    softmax('fp32', {}, dt=f32)
    softmax('EMO_SATTN32=0', {'EMO_SATTN32': '0'})
    softmax('EMO_SATTN32_BWD=0', {'EMO_SATTN32_BWD': '0'})
    softmax('EMO_SATTN32_DQ=0', {'EMO_SATTN32_DQ': '0'})

    lens = torch.tensor([1, 17, 45], dtype=torch.int64, device='cuda')
    for tag, env, T_max in (('1024 threads', {}, 45), ('EMO_SATTN_DECODE_NT=256', {'EMO_SATTN_DECODE_NT': '256'}, 45), ('T_max * 4 > 96 KB', {}, 24600)):
        kc, vc = rnd(n, T_max, HD, dt=bf), rnd(n, T_max, HD, dt=bf)
        out.append(('softmax decode ' + tag, env, lambda kc=kc, vc=vc: ops.softmax_attn_decode(qd, kc, vc, lens, H, k_new=kd, v_new=vd)))

    T, T_max = 70, 45
    for dt, name in ((f32, 'fp32'), (bf, 'bf16')):
        qkv, dout = rnd(B * T, 3 * HD, dt=dt), rnd(B * T, HD, dt=dt)
        q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
        R, u, vb = rnd(T, HD, dt=dt), rnd(H, dh) * 0.4, rnd(H, dh) * 0.4
        fwd = lambda w, q=q, k=k, v=v, R=R, u=u, vb=vb: ops.relpos_attn_fwd(q, k, v, R, u, vb, B, T, H, window=w)
        o, lse, zden = fwd(0)
        for w in (0, 8, T - 1):
            out.append(('relpos fwd %s window %d' % (name, w), {}, lambda w=w, fwd=fwd: fwd(w)))
        dqkv, dq_rel, delta = torch.empty_like(qkv), torch.empty_like(o), torch.empty_like(lse)
        dR, (qu, qv) = torch.empty(T, HD, device='cuda'), ops.add_bias2(q, u, vb)
        ws, ws_bytes = ops._workspace('relpos_dr', qkv.device, ops.lib.emo_relpos_attn_bwd_r_workspace_bytes(B, T, H, dh))
        common = dict(r_dist=ptr(R), ld_r=_rows(R), n_dist=T, dout=ptr(dout), ld_out=HD, lse=ptr(lse), zden=ptr(zden), delta=ptr(delta), ld_d=3 * HD)
        back = dict(common, qu=ptr(qu), qv=ptr(qv), ld_q=HD)
        keep_alive = (qkv, dout, R, u, vb, o, lse, zden, dqkv, dq_rel, delta, dR, qu, qv, ws)
        out.append(('relpos bwd ' + name, {}, lambda q=q, k=k, v=v, u=u, vb=vb, o=o, dqkv=dqkv, dq_rel=dq_rel, common=common, _=keep_alive: _attn(
            ATTN_RELPOS, ATTN_BWD, q, k, v, B, T, H, r_w_bias=ptr(u), r_r_bias=ptr(vb), out=ptr(o), dq=ptr(dqkv), dq_rel=ptr(dq_rel), ld_rel=HD, **common)))
        out.append(('relpos bwd_kv ' + name, {}, lambda k=k, v=v, qu=qu, dqkv=dqkv, back=back: _attn(
            ATTN_RELPOS, ATTN_BWD_KV, qu, k, v, B, T, H, dk=ptr(dqkv[:, HD:2 * HD]), dv=ptr(dqkv[:, 2 * HD:]), **back)))
        out.append(('relpos bwd_r ' + name, {}, lambda k=k, v=v, qu=qu, dR=dR, ws=ws, ws_bytes=ws_bytes, back=back: _attn(
            ATTN_RELPOS, ATTN_BWD_R, qu, k, v, B, T, H, dR=ptr(dR), ld_dr=HD, workspace=ptr(ws), workspace_bytes=ws_bytes, **back)))
        rowd = rnd(n, 3 * HD, dt=dt)
        kc, vc, Rd = rnd(n, T_max, HD, dt=dt), rnd(n, T_max, HD, dt=dt), rnd(T_max, HD, dt=dt)
        out.append(('relpos decode ' + name, {}, lambda rowd=rowd, kc=kc, vc=vc, Rd=Rd, u=u, vb=vb: ops.relpos_attn_decode(
            rowd[:, :HD], kc, vc, lens, H, Rd, u, vb, k_new=rowd[:, HD:2 * HD], v_new=rowd[:, 2 * HD:])))
    return out


def run(label_file):
    import torch
    from emo_disentanger_amd import ops
    for name in SWITCHES:
        os.environ.pop(name, None)
    todo = cases()
    gauss, omega = torch.randn(1, 1, 16, 16, device='cuda'), torch.empty(1, 16, 16, device='cuda')
    torch.cuda.synchronize()
    done = open(label_file, 'w')
    for label, env, thunk in todo:
        os.environ.update(env)
        ops.favor_draw_omega(gauss, omega)
        thunk()
        torch.cuda.synchronize()
        for name in env:
            del os.environ[name]
        done.write(label + '\n')
        done.flush()
    ops.favor_draw_omega(gauss, omega)
    torch.cuda.synchronize()


def names(trace, label_file):
    rows = list(csv.DictReader(open(trace)))
    col = lambda want: next(c for c in rows[0] if c.lower() == want)
    kn, ts = col('kernel_name'), col('start_timestamp')
    rows.sort(key=lambda r: int(r[ts]))
    short = [re.sub(r'\(.*', '', r[kn].replace('(anonymous namespace)::', '').replace('void ', '')) for r in rows]
    groups, cur = [], None
    for s in short:
        if s.startswith(SEPARATOR):
            cur = []
            groups.append(cur)
        elif cur is not None:
            cur.append(s)
    groups = groups[:-1]                                       # (the last separator closes the last case)
    lab = [l.rstrip('\n') for l in open(label_file) if l.strip()]
    assert len(lab) == len(groups), 'labels %d vs separator groups %d' % (len(lab), len(groups))
    print(json.dumps(dict(zip(lab, groups)), indent=1))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--names':
        names(sys.argv[2], sys.argv[3])
    else:
        run(sys.argv[1])
