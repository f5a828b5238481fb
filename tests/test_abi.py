"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol that
include/emo_hip.h declares; argument validation errors surface as Python exceptions (no compute)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, 'include', 'emo_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(emo_[a-z0-9_]+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    from emo_disentanger_amd import _lib
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(_lib.lib, n), 'libemo_hip.so does not export %s' % n
        assert n in _lib._SIG, 'ctypes signature missing for %s' % n
    assert set(_lib._SIG) == set(names)
    assert _lib.lib.emo_version() >= 100


def test_invalid_arguments_raise_without_a_gpu():
    from emo_disentanger_amd import _lib
    rc = _lib.lib.emo_gemm(None, 0, 8, None, 0, 8, None, 8, 4, 4, 4, 1, 1, 0, None, None)
    assert rc == -1 and b'null pointer' in _lib.lib.emo_last_error()
    with pytest.raises(_lib.EmoError):
        _lib.check(rc)
    import torch
    with pytest.raises(_lib.EmoError):
        _lib.ptr(torch.zeros(3))           # CPU tensor: the product path has no CPU fallback
    with pytest.raises(_lib.EmoError):
        _lib.dtype_code(torch.float16)


def test_epilogue_struct_mirror_has_the_library_size():
    # the ctypes mirror of emo_epilogue_t (fields are appended as epilogue features are added) must match the struct the library was built with
    import ctypes
    from emo_disentanger_amd import _lib
    assert _lib.lib.emo_epilogue_size() == ctypes.sizeof(_lib.Epilogue)


def test_decode_step_struct_mirror_has_the_library_size():
    # the ctypes mirror of emo_decode_step_t, as for emo_epilogue_t above: a stale mirror would hand the launch garbage addresses
    from emo_disentanger_amd import _lib
    assert _lib.lib.emo_decode_step_size() == ctypes.sizeof(_lib.DecodeStep)


_FORM_NAME = {0: 'performer', 1: 'gpt2', 2: 'txl'}


def _decode_step_args(form, **kw):
    """A block that passes every host check of `form` (pointer fields: small fake addresses, 16-byte aligned — validation never dereferences them,
    and no refusal below gets as far as the device query or the launch), with the fields of `kw` changed."""
    from emo_disentanger_amd import _lib
    a = _lib.DecodeStep()
    for name, ctype in _lib.DecodeStep._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.form, a.sampled, a.n_layers, a.n_token, a.n_streams, a.n_real = form, 0, 2, 327, 4, 4
    a.d_model, a.n_head, a.n_feat, a.d_ff = 512, 8, 128, 2048
    a.sync_ws_bytes = _lib.lib.emo_decode_step_workspace_bytes()
    a.temperature, a.top_p, a.emb_scale, a.eps, a.ln_eps = 1.0, 0.9, 1.0, 1e-6, 1e-5
    a.kv_tmax, a.mem_len, a.n_dist = 2048, 64, 65
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('form, sampled, kw, what', [
    (0, 0, dict(d_model=256), 'built for d_model 512'), (1, 0, dict(d_model=256), 'built for d_model 512'), (2, 0, dict(d_model=256), 'built for d_model 512'),
    (0, 0, dict(n_streams=6), 'multiple of 4'), (1, 0, dict(n_streams=6), 'multiple of 4'), (2, 0, dict(n_streams=6), 'multiple of 4'),
    (1, 0, dict(kv_tmax=4096), 'KV cache of <= 2048 rows'),
    (2, 0, dict(mem_len=2048), '1 <= mem_len and mem_len + 1 <= 2048 (got mem_len 2048)'),
    (2, 0, dict(mem_len=64, n_dist=64), 'the R tables have 64 rows, the window reaches distance 64'),
    (0, 1, dict(temperature=0.0), 'bad sampling arguments'), (1, 1, dict(temperature=0.0), 'bad sampling arguments'),
])
def test_decode_step_refuses_bad_arguments_without_a_gpu_and_names_its_form(form, sampled, kw, what):
    from emo_disentanger_amd import _lib
    a = _decode_step_args(form, sampled=sampled, **kw)
    assert _lib.lib.emo_decode_step(ctypes.byref(a), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert what in msg
    assert msg.startswith('emo_decode_step[%s%s]: ' % (_FORM_NAME[form], ', sampled' if sampled else ''))
    with pytest.raises(_lib.EmoError):
        _lib.check(-1)


def test_decode_step_refuses_an_all_zero_block_without_a_gpu():
    from emo_disentanger_amd import _lib
    a = _lib.DecodeStep()
    assert _lib.lib.emo_decode_step(ctypes.byref(a), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert msg.startswith('emo_decode_step[performer]: ') and 'null pointer' in msg
    assert _lib.lib.emo_decode_step(None, None) == -1 and b'null argument block' in _lib.lib.emo_last_error()


def test_grammar_step_struct_mirror_has_the_library_size():
    # the ctypes mirror of emo_grammar_step_t, as for the two structs above
    from emo_disentanger_amd import _lib
    assert _lib.lib.emo_grammar_step_size() == ctypes.sizeof(_lib.GrammarStep)


_KIND_NAME = {0: 'txl', 1: 'acc', 2: 'acc_window'}


def _grammar_step_args(kind, **kw):
    """A block that passes every host check of `kind` (pointer fields: small fake addresses, 16-byte aligned — validation never dereferences
    them, and no refusal below gets as far as the launch), with the fields of `kw` changed."""
    from emo_disentanger_amd import _lib
    a = _lib.GrammarStep()
    for name, ctype in _lib.GrammarStep._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.kind, a.n_rows, a.n_token, a.n_u, a.ld_u, a.ld_seq, a.max_len, a.window = kind, 3, 327, 8, 3, 64, 32, 32
    a.temperature, a.top_p, a.key_temperature, a.key_top_p = 1.2, 0.9, 1.1, 0.97
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('kind, kw, what', [
    (0, dict(n_token=2000), 'V must be <= 1024 (got 2000)'), (1, dict(n_token=2000), 'V must be <= 1024 (got 2000)'),
    (2, dict(n_token=2000), 'V must be <= 1024 (got 2000)'),
    (0, dict(temperature=0.0), 'temperatures must be > 0'), (1, dict(temperature=0.0), 'temperature must be > 0'),
    (2, dict(temperature=0.0), 'temperature must be > 0'),
    (0, dict(key_temperature=0.0), 'temperatures must be > 0'),
    (2, dict(window=65), 'bad sizes'),
    (0, dict(tok_out=None), 'null pointer'), (1, dict(seg_out=None), 'null pointer'), (2, dict(win_seg=None), 'null pointer'),
    (1, dict(max_len=0), 'bad sizes'), (0, dict(ld_u=2), 'bad sizes'),
])
def test_grammar_step_refuses_bad_arguments_without_a_gpu_and_names_its_kind(kind, kw, what):
    from emo_disentanger_amd import _lib
    a = _grammar_step_args(kind, **kw)
    assert _lib.lib.emo_grammar_step(ctypes.byref(a), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert what in msg
    assert msg.startswith('emo_grammar_step[%s]: ' % _KIND_NAME[kind])
    with pytest.raises(_lib.EmoError):
        _lib.check(-1)


def test_grammar_step_refuses_an_empty_a_missing_and_an_unknown_block_without_a_gpu():
    from emo_disentanger_amd import _lib
    a = _lib.GrammarStep()
    assert _lib.lib.emo_grammar_step(ctypes.byref(a), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert msg.startswith('emo_grammar_step[txl]: ') and 'null pointer' in msg
    assert _lib.lib.emo_grammar_step(None, None) == -1 and b'null argument block' in _lib.lib.emo_last_error()
    assert _lib.lib.emo_grammar_step(ctypes.byref(_grammar_step_args(7)), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert msg.startswith('emo_grammar_step: ') and 'kind 7' in msg


def test_a_kind_ignores_the_fields_of_the_other_kinds():
    # a block is refused for its own kind's fields only: the windowed kind's NULL win_tok does not stop TXL or ACC getting past the pointer
    # check (each goes on to its next refusal, a size of its own)
    from emo_disentanger_amd import _lib
    for kind, kw in ((0, dict(segs=None, lead_tok=None, seg_out=None, rows=None, win_tok=None, win_seg=None, max_len=0, window=0)),
                     (1, dict(rows=None, win_tok=None, win_seg=None, window=0, key_temperature=0.0)),
                     (2, dict(rows=None, tok_out=None, seg_out=None, max_len=0, key_temperature=0.0))):
        a = _grammar_step_args(kind, n_u=0, **kw)
        assert _lib.lib.emo_grammar_step(ctypes.byref(a), None) == -1
        assert _lib.lib.emo_last_error().decode() == 'emo_grammar_step[%s]: bad sizes' % _KIND_NAME[kind]


def test_attn_struct_mirror_has_the_library_size():
    # the ctypes mirror of emo_attn_t, as for the three structs above
    from emo_disentanger_amd import _lib
    assert _lib.lib.emo_attn_size() == ctypes.sizeof(_lib.Attn)


_ATTN_KIND = {0: 'favor', 1: 'softmax', 2: 'relpos'}
_ATTN_PASS = {0: 'fwd', 1: 'bwd', 2: 'bwd_kv', 3: 'bwd_r', 4: 'decode'}
_ATTN_PASSES = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (2, 3), (0, 4), (1, 4), (2, 4)]          # every (kind, pass) the entry has


def _attn_args(kind, pass_, **kw):
    """A block that passes every host check of its (kind, pass) (pointer fields: small fake addresses, 16-byte aligned — validation never
    dereferences them; such a block would go on to the launch, so every caller breaks one field), with the fields of `kw` changed.
    bf16, B * H = 256 single-segment FAVOR scans (the dout_is_dn class), T = 128 with dropout (the class that has keep words); the DECODE pass:
    T = 1 against caches of T_max = 128 rows, no window."""
    from emo_disentanger_amd import _lib
    a = _lib.Attn()
    for name, ctype in _lib.Attn._fields_:
        if ctype is _lib.c_p:
            setattr(a, name, 0x1000)
    a.kind, a.pass_, a.dtype, a.B, a.T, a.H, a.dh, a.n_feat = kind, pass_, _lib.BF16, 32, 128, 8, 64, 128
    a.ld, a.ld_out, a.ld_d, a.ld_r, a.n_dist, a.ld_rel, a.ld_q, a.ld_dr = 1536, 512, 1536, 512, 128, 512, 512, 512
    a.p_drop, a.seed, a.offset, a.eps = 0.1, 7, 3, 1e-6
    a.keep_bytes = _lib.lib.emo_softmax_attn_keep_bytes(_lib.BF16, 32, 128, 8, 64, 0.1)
    a.workspace_bytes = _lib.lib.emo_relpos_attn_bwd_r_workspace_bytes(32, 128, 8, 64)
    assert a.keep_bytes > 0 and a.workspace_bytes > 0
    if pass_ == 4:
        a.T, a.T_max, a.lens_off, a.window = 1, 128, 0, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize('kind, pass_, kw, what', [
    (0, 0, dict(omega=None), 'null pointer'), (0, 0, dict(n_feat=127), 'n_feat must be even'), (0, 0, dict(workspace=0x1008), 'workspace must be 16-B aligned'),
    (0, 1, dict(den=None), 'null pointer'), (0, 1, dict(ld_d=1538), 'ld_d must be a multiple of 4'), (0, 1, dict(ld=1540), 'ld/dh must keep rows 16-B aligned'),
    (0, 1, dict(dout_is_dn=1, dq=None), 'null pointer'), (0, 1, dict(dout_is_dn=1, B=4, T=1024), 'dout_is_dn outside its class'),      # B * H = 32: a segmented scan
    (0, 1, dict(dout_is_dn=1, dtype=0), 'dout_is_dn outside its class'),
    (1, 0, dict(lse=None), 'bad out/lse'), (1, 0, dict(ld=1540), 'ld/dh must keep rows 16-B aligned'), (1, 0, dict(keep_bytes=1024), 'keep buffer of 1024 bytes'),
    (1, 1, dict(delta_ws=None), 'null pointer'), (1, 1, dict(ld_d=1538), 'ld_d % 4 == 0'), (1, 1, dict(keep_bytes=1024), 'keep buffer of 1024 bytes'),
    (1, 1, dict(dtype=3), 'bad dtype'),
    (2, 0, dict(r_dist=None), 'null pointer'), (2, 0, dict(n_dist=127), 'a row for every distance'), (2, 0, dict(ld_r=516), 'r_dist must keep rows 16-B aligned'),
    (2, 1, dict(dq_rel=None), 'null pointer'), (2, 1, dict(ld_rel=510), 'ld_rel % 4 == 0'), (2, 1, dict(q=None), 'null pointer'),
    (2, 2, dict(qv=None), 'null pointer'), (2, 2, dict(ld_d=1538), 'ld_d % 4 == 0'), (2, 2, dict(qu=None), 'null pointer'), (2, 2, dict(ld_q=516), 'qu / qv / dout'),
    (2, 3, dict(dR=None), 'dR / workspace'), (2, 3, dict(workspace_bytes=1024), 'workspace too small'), (2, 3, dict(ld_dr=256), 'a column for every (h, d)'),
    (0, 4, dict(state_z=None), 'null pointer'), (0, 4, dict(k=None), 'null pointer'), (0, 4, dict(dh=48), 'd_head<=64 dividing 256'),
    (0, 4, dict(n_feat=256), 'n_feat<=128'), (0, 4, dict(T=2), 'T must be 1'), (0, 4, dict(window=8), 'window > 0 is served by [relpos, fwd] and [relpos, decode] only'),
    (1, 4, dict(kcache=None), 'null pointer'), (1, 4, dict(v=None), 'go together'), (1, 4, dict(T_max=40000), 'T_max too large for the LDS score buffer'),
    (1, 4, dict(kcache=0x1008), 'caches must be 16-B aligned'), (1, 4, dict(dh=48), 'd_head must be 16, 32, 64 or 128'), (1, 4, dict(T=128), 'T must be 1'),
    (1, 4, dict(window=8), 'window > 0 is served by [relpos, fwd] and [relpos, decode] only'),
    (2, 4, dict(r_w_bias=None), 'null pointer'), (2, 4, dict(n_dist=127), 'a row for every distance 0 .. T_max-1'), (2, 4, dict(ld_r=516), 'caches / r_dist must be 16-B aligned'),
    (2, 4, dict(k=None), 'go together'), (2, 4, dict(T_max=40000, n_dist=40000), 'T_max too large for the LDS score buffer'), (2, 4, dict(dtype=3), 'bad dtype'),
    (0, 4, dict(n_feat=127), 'n_feat must be even'),             # (the shared FAVOR check runs in front of the DECODE pass too)
])
def test_attn_refuses_bad_arguments_without_a_gpu_and_names_its_kind_and_pass(kind, pass_, kw, what):
    from emo_disentanger_amd import _lib
    a = _attn_args(kind, pass_, **kw)
    assert _lib.lib.emo_attn(ctypes.byref(a), None) == -1          # (-1: a host refusal; a HIP call on this machine would come back as -2)
    msg = _lib.lib.emo_last_error().decode()
    assert what in msg
    assert msg.startswith('emo_attn[%s, %s%s]: ' % (_ATTN_KIND[kind], _ATTN_PASS[pass_], ', dn' if a.dout_is_dn else ''))
    with pytest.raises(_lib.EmoError):
        _lib.check(-1)


def test_attn_refusal_cases_cover_every_kind_and_pass():
    cases = test_attn_refuses_bad_arguments_without_a_gpu_and_names_its_kind_and_pass.pytestmark[0].args[1]
    assert {(c[0], c[1]) for c in cases} == set(_ATTN_PASSES)


def test_attn_refuses_an_empty_a_missing_and_an_unknown_block_without_a_gpu():
    from emo_disentanger_amd import _lib
    a = _lib.Attn()
    assert _lib.lib.emo_attn(ctypes.byref(a), None) == -1
    assert _lib.lib.emo_last_error().decode() == 'emo_attn[favor, fwd]: null pointer'
    assert _lib.lib.emo_attn(None, None) == -1 and b'emo_attn: null argument block' in _lib.lib.emo_last_error()
    assert _lib.lib.emo_attn(ctypes.byref(_attn_args(3, 0)), None) == -1
    msg = _lib.lib.emo_last_error().decode()
    assert msg.startswith('emo_attn: ') and 'kind 3' in msg
    for kind, pass_ in ((0, 2), (1, 3), (2, 5), (0, 5), (0, -1)):   # BWD_KV / BWD_R are passes of RELPOS only; DECODE (4) is the last pass of every kind
        assert _lib.lib.emo_attn(ctypes.byref(_attn_args(kind, pass_)), None) == -1
        msg = _lib.lib.emo_last_error().decode()
        assert msg == 'emo_attn: kind %s has no pass %d' % (_ATTN_KIND[kind], pass_)


def test_an_attention_kind_ignores_the_fields_of_the_other_kinds_and_passes():
    # a block is refused for the fields of its own (kind, pass) only: with every other kind's and pass's fields NULL / zero it gets as far as the
    # LAST host check of its own, which one broken field of its own then fails
    favor = dict(omega=None, den=None, state_S=None, state_z=None, n_feat=1, eps=0.0, kstate_valid=1, dout_is_dn=0)
    softmax = dict(delta_ws=None, keep=None, keep_bytes=0)
    relpos = dict(r_dist=None, ld_r=1, n_dist=0, r_w_bias=None, r_r_bias=None, zden=None, dq_rel=None, ld_rel=1, delta=None, qu=None, qv=None, ld_q=1, dR=None,
                  ld_dr=0)
    bwd = dict(dout=None, dq=None, dk=None, dv=None, ld_d=1)
    cache = dict(kcache=None, vcache=None, T_max=0, lens=None, lens_off=0, head_major=0)      # the DECODE passes' own: FWD and the backward passes ignore them
    # what no DECODE pass reads: the gradients, the statistics, dropout, the scratch buffers, the biased query copies
    train = dict(bwd, workspace=None, workspace_bytes=0, den=None, kstate_valid=0, dout_is_dn=0, lse=None, zden=None, dq_rel=None, ld_rel=1, delta=None, qu=None,
                 qv=None, ld_q=1, dR=None, ld_dr=0, p_drop=0.0, seed=0, offset=0, **softmax)
    relpos_in = dict(r_dist=None, ld_r=1, n_dist=0, r_w_bias=None, r_r_bias=None)
    for kind, pass_, others, broken, what in (
            (0, 0, dict(softmax, lse=None, **relpos, **bwd, **cache), dict(state_z=None), 'state_S without state_z'),
            (0, 1, dict(softmax, lse=None, **relpos, **cache), dict(dout_is_dn=1, den=None, workspace=None, dv=0x1008), 'pointers must be 16-B aligned'),
            (1, 0, dict(favor, workspace=None, **relpos, **bwd, **cache), dict(keep_bytes=16), 'keep buffer of 16 bytes'),
            (1, 1, dict(favor, workspace=None, **relpos, **cache), dict(keep_bytes=16), 'keep buffer of 16 bytes'),
            (2, 0, dict(favor, workspace=None, **softmax, **bwd, **cache, qu=None, qv=None, dq_rel=None, dR=None, delta=None, zden=None), dict(out=0x1008),
             'out must be 16-B aligned'),
            (2, 1, dict(favor, workspace=None, **softmax, **cache, dk=None, dv=None, qu=None, qv=None, dR=None, delta=None), dict(ld_rel=510), 'ld_rel % 4 == 0'),
            (2, 2, dict(favor, workspace=None, **softmax, **cache, q=None, out=None, dq=None, dq_rel=None, dR=None, r_w_bias=None, r_r_bias=None), dict(ld_d=1538),
             'ld_d % 4 == 0'),
            (2, 3, dict(favor, **softmax, **cache, q=None, out=None, dq=None, dk=None, dv=None, ld_d=1, dq_rel=None, r_w_bias=None, r_r_bias=None),
             dict(workspace_bytes=16), 'workspace too small'),
            (0, 4, dict(train, **relpos_in, **cache), dict(dh=48), 'needs 16<=d_head<=64 dividing 256'),
            (1, 4, dict(train, **relpos_in, omega=None, state_S=None, state_z=None, n_feat=1, eps=0.0), dict(T_max=40000), 'T_max too large for the LDS score buffer'),
            (2, 4, dict(train, omega=None, state_S=None, state_z=None, n_feat=1, eps=0.0, head_major=1), dict(ld_r=516), 'caches / r_dist must be 16-B aligned')):
        from emo_disentanger_amd import _lib
        a = _attn_args(kind, pass_, **dict(others, **broken))
        assert _lib.lib.emo_attn(ctypes.byref(a), None) == -1
        msg = _lib.lib.emo_last_error().decode()
        assert msg.startswith('emo_attn[%s, %s%s]: ' % (_ATTN_KIND[kind], _ATTN_PASS[pass_], ', dn' if a.dout_is_dn else '')) and what in msg, msg
