"""ctypes binding of libemo_hip.so (C-ABI declared in include/emo_hip.h).

The library is built IN-TREE by ``__graft_entry__.build()`` / ``make -C emo-disentanger_amd/csrc``.
Missing library => ImportError (the product path has no CPU / eager fallback)."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libemo_hip.so')

F32, BF16, I64 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_GELU_NEW, ACT_GELU = 0, 1, 2, 3
MUL_NONE, MUL_NONZERO, MUL_DGELU_NEW, MUL_BITMASK, MUL_DGELU = 0, 1, 2, 3, 4

if not os.path.exists(LIB_PATH):
    raise ImportError('libemo_hip.so not built: run `python -c "import __graft_entry__ as g; g.build()"` '
                      'or `make -C emo-disentanger_amd/csrc` (hipcc --offload-arch=gfx950)')
lib = ctypes.CDLL(LIB_PATH)

c_p, c_i, c_l, c_f, c_u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64


class Epilogue(ctypes.Structure):
    _fields_ = [('bias', c_p), ('act', c_i), ('aux_out', c_p), ('mul_aux', c_p), ('mul_mode', c_i), ('mul_scale', c_f),
                ('p_drop', c_f), ('seed', c_u64), ('offset', c_u64), ('residual', c_p),
                ('ln_c1', c_p), ('ln_eps', c_f), ('ln_stats_out', c_p), ('rln_x', c_p), ('rln_stats', c_p), ('rln_gamma', c_p), ('rln_beta', c_p), ('a_rowsum', c_p), ('b_rowsum', c_p),
                ('mask_out', c_p), ('workspace', c_p), ('workspace_bytes', c_l),
                ('lna_gamma', c_p), ('lna_beta', c_p), ('lna_out', c_p), ('lna_mean', c_p), ('lna_rstd', c_p), ('hdiv', c_p), ('hdiv_T', c_l)]


class DecodeStep(ctypes.Structure):
    """emo_decode_step_t (emo_hip.h), field for field: the argument block of the one-launch token step.  Pointer fields hold raw device addresses."""
    _fields_ = [('form', ctypes.c_int32), ('sampled', ctypes.c_int32), ('layer_table', c_p), ('n_layers', c_l),
                ('tok', c_p), ('seg', c_p), ('E', c_p), ('Sg', c_p), ('pe', c_p), ('emb_scale', c_f), ('pos0', c_l), ('pos_ids', c_p),
                ('wout_packed', c_p), ('bout', c_p), ('n_token', c_l), ('logits', c_p),
                ('n_streams', c_l), ('n_real', c_l), ('d_model', c_l), ('n_head', c_l), ('n_feat', c_l), ('d_ff', c_l),
                ('sync_ws', c_p), ('sync_ws_bytes', c_l), ('eps', c_f), ('ln_eps', c_f), ('diag', c_p),
                ('temperature', c_f), ('top_p', c_f), ('u_steps', c_p), ('step', c_p), ('seq', c_p), ('ld_seq', c_l), ('col0', c_l), ('tok_out', c_p),
                ('ln0', c_p), ('kv_tmax', c_l), ('lens', c_p), ('mem_len', c_l), ('n_dist', c_l), ('r_w_bias', c_p), ('r_r_bias', c_p)]


class GrammarStep(ctypes.Structure):
    """emo_grammar_step_t (emo_hip.h), field for field: the argument block of the five device grammar steps.  Pointer fields hold raw device addresses."""
    _fields_ = [('kind', ctypes.c_int32), ('n_rows', c_l), ('logits', c_p), ('n_token', c_l), ('temperature', c_f), ('top_p', c_f),
                ('u_steps', c_p), ('n_u', c_l), ('ld_u', c_l), ('ev_flags', c_p), ('ev_beat', c_p), ('params', c_p), ('state', c_p),
                ('seq', c_p), ('ld_seq', c_l), ('running', c_p),
                ('key_temperature', c_f), ('key_top_p', c_f), ('tok_out', c_p), ('seg_out', c_p), ('max_len', c_l), ('pad', c_l),
                ('guide_cond', c_p), ('guide_uncond', c_p), ('guide_scale', c_p),
                ('segs', c_p), ('lead_tok', c_p), ('lead_off', c_p),
                ('keep_tok', c_p), ('keep_beg', c_p), ('keep_end', c_p), ('n_keep', c_l), ('keep_eos', c_l), ('keep_bar', c_l), ('keep_left', c_p), ('track_full', c_l), ('window', c_l), ('rows', c_p), ('win_tok', c_p), ('win_seg', c_p),
                ('tok_bias', c_p), ('n_biases', c_l), ('bias_of', c_p), ('top_k_of', c_p), ('min_p_of', c_p),
                ('slot_job', c_p), ('queue_head', c_p), ('n_jobs', c_l), ('mem_lens', c_p), ('mem_rows', c_l), ('job_steps', c_p),
                ('tok_mask', c_p), ('n_masks', c_l), ('mask_of', c_p), ('temp_of', c_p), ('top_p_of', c_p), ('row_reset', c_p),
                ('tok_logp', c_p), ('tok_rank', c_p), ('tok_entropy', c_p)]


class AccRebase(ctypes.Structure):
    """emo_acc_rebase_t (emo_hip.h), field for field: the argument block of the re-anchoring launch.  Pointer fields hold raw device addresses."""
    _fields_ = [('n_rows', c_l), ('seq', c_p), ('segs', c_p), ('ld_seq', c_l), ('state', c_p), ('params', c_p), ('primer_len', c_p),
                ('track_leadsheet', c_l), ('keep', c_l), ('window', c_l), ('longest_bar', c_l), ('pad', c_l),
                ('dst_seq', c_p), ('dst_segs', c_p), ('ld_dst', c_l), ('arch_tok', c_p), ('arch_len', c_p), ('ld_arch', c_l),
                ('tok_logp', c_p), ('tok_rank', c_p), ('tok_entropy', c_p), ('dst_logp', c_p), ('dst_rank', c_p), ('dst_entropy', c_p),
                ('arch_logp', c_p), ('arch_rank', c_p), ('arch_entropy', c_p), ('new_len', c_p), ('running', c_p)]


GRAMMAR_TXL, GRAMMAR_ACC, GRAMMAR_ACC_WINDOW, GRAMMAR_TXL_QUEUE, GRAMMAR_ACC_QUEUE = 0, 1, 2, 3, 4      # emo_hip.h: EMO_GRAMMAR_*


class Attn(ctypes.Structure):
    """emo_attn_t (emo_hip.h), field for field: the argument block of the attention kernels (training passes and the one-token DECODE pass).
    Pointer fields hold raw device addresses."""
    _fields_ = [('kind', ctypes.c_int32), ('pass_', ctypes.c_int32),
                ('q', c_p), ('k', c_p), ('v', c_p), ('ld', c_l), ('out', c_p), ('dout', c_p), ('ld_out', c_l), ('dq', c_p), ('dk', c_p), ('dv', c_p), ('ld_d', c_l),
                ('dtype', ctypes.c_int32), ('B', c_l), ('T', c_l), ('H', c_l), ('dh', c_l), ('p_drop', c_f), ('seed', c_u64), ('offset', c_u64),
                ('workspace', c_p), ('workspace_bytes', c_l),
                ('omega', c_p), ('den', c_p), ('state_S', c_p), ('state_z', c_p), ('n_feat', c_l), ('eps', c_f), ('kstate_valid', ctypes.c_int32), ('dout_is_dn', ctypes.c_int32),
                ('lse', c_p), ('delta_ws', c_p), ('keep', c_p), ('keep_bytes', c_l),
                ('r_dist', c_p), ('ld_r', c_l), ('n_dist', c_l), ('r_w_bias', c_p), ('r_r_bias', c_p), ('zden', c_p), ('dq_rel', c_p), ('ld_rel', c_l), ('delta', c_p),
                ('qu', c_p), ('qv', c_p), ('ld_q', c_l), ('dR', c_p), ('ld_dr', c_l), ('window', c_l),
                ('kcache', c_p), ('vcache', c_p), ('T_max', c_l), ('lens', c_p), ('lens_off', c_l), ('head_major', ctypes.c_int32)]


ATTN_FAVOR, ATTN_SOFTMAX, ATTN_RELPOS = 0, 1, 2             # emo_hip.h: EMO_ATTN_* kinds
ATTN_FWD, ATTN_BWD, ATTN_BWD_KV, ATTN_BWD_R, ATTN_DECODE = 0, 1, 2, 3, 4    # ... and passes (`pass` is a Python keyword: the mirror's field is pass_)

_SIG = {
    'emo_version': (c_i, []),
    'emo_build_flags': (c_i, []),
    'emo_last_error': (ctypes.c_char_p, []),
    'emo_device_cus': (c_i, []),
    'emo_gemm': (c_i, [c_p, c_i, c_l, c_p, c_i, c_l, c_p, c_l, c_l, c_l, c_l, c_i, c_i, c_i, ctypes.POINTER(Epilogue), c_p]),
    'emo_gemm_route': (c_i, [c_p, c_i, c_l, c_p, c_i, c_l, c_p, c_l, c_l, c_l, c_l, c_i, c_i, c_i, ctypes.POINTER(Epilogue), ctypes.POINTER(c_i), ctypes.POINTER(c_i)]),
    'emo_gemm_astat_supported': (c_i, [c_i, c_i, c_l, c_l, c_l]),
    'emo_gemm_astat_min_rows': (c_l, []),
    'emo_gemm_last_kernel': (c_i, []),
    'emo_gemm_last_plan': (c_i, []),
    'emo_epilogue_size': (c_i, []),
    'emo_gemm_workspace_bytes': (c_l, [c_l, c_l, c_l, c_i, c_i]),
    'emo_ffn_fwd_supported': (c_i, [c_i, c_l, c_l, c_l]),
    'emo_ffn_fwd': (c_i, [c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_l, c_l, c_l, c_i, c_f, c_u64, c_u64, c_u64, c_p]),
    'emo_colsum': (c_i, [c_p, c_i, c_l, c_l, c_l, c_p, c_i, c_p]),
    'emo_embed_fwd': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_l, c_l, c_l, c_l, c_l, c_l, c_p, c_f, c_f, c_u64, c_u64, c_p]),
    'emo_embed_bwd': (c_i, [c_p, c_p, c_p, c_i, c_p, c_p, c_l, c_l, c_l, c_l, c_l, c_f, c_f, c_u64, c_u64, c_p]),
    'emo_layernorm_fwd': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_l, c_l, c_f, c_p]),
    'emo_layernorm_bwd': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_l, c_l, c_f, c_u64, c_u64, c_p, c_l, c_p]),
    'emo_layernorm_bwd_workspace_bytes': (c_l, [c_i, c_l, c_l]),
    'emo_dropout_apply': (c_i, [c_p, c_p, c_i, c_l, c_f, c_u64, c_u64, c_p]),
    'emo_attn_size': (c_i, []),
    'emo_attn': (c_i, [ctypes.POINTER(Attn), c_p]),
    'emo_favor_attn_workspace_bytes': (c_l, [c_l, c_l, c_l, c_l, c_l]),
    'emo_favor_attn_bwd_dn_supported': (c_i, [c_i, c_l, c_l, c_l, c_l, c_l]),
    'emo_decode_step_size': (c_i, []),
    'emo_decode_step_workspace_bytes': (c_l, []),
    'emo_decode_step_supported': (c_i, []),
    'emo_decode_step': (c_i, [ctypes.POINTER(DecodeStep), c_p]),
    'emo_favor_draw_omega': (c_i, [c_p, c_p, c_l, c_l, c_l, c_p]),
    'emo_favor_state_reset': (c_i, [c_p, c_l, c_l, c_l, c_l, c_p, c_p]),
    'emo_favor_state_at': (c_i, [c_p, c_p, c_l, c_i, c_p, c_p, c_p, c_p, c_l, c_l, c_l, c_l, c_l, c_p]),
    'emo_softmax_attn_keep_bytes': (c_l, [c_i, c_l, c_l, c_l, c_l, c_f]),
    'emo_relpos_attn_bwd_r_workspace_bytes': (c_l, [c_l, c_l, c_l, c_l]),
    'emo_xent_fwd': (c_i, [c_p, c_p, c_l, c_l, c_l, c_p, c_p, c_p]),
    'emo_xent_bwd': (c_i, [c_p, c_p, c_p, c_p, c_p, c_l, c_i, c_l, c_l, c_l, c_p]),
    'emo_token_scores': (c_i, [c_p, c_l, c_p, c_l, c_l, c_l, c_p, c_p, c_p, c_p, c_p]),
    'emo_xent_bwd_rows': (c_i, [c_p, c_l, c_p, c_p, c_p, c_p, c_l, c_i, c_l, c_l, c_l, c_p]),
    'emo_argmax': (c_i, [c_p, c_l, c_l, c_p, c_p]),
    'emo_sample_nucleus': (c_i, [c_p, c_l, c_l, c_f, c_f, c_p, c_p, c_p]),
    'emo_sample_nucleus_step': (c_i, [c_p, c_l, c_l, c_f, c_f, c_p, c_p, c_p, c_l, c_l, c_p, c_p]),
    'emo_grammar_step_size': (c_i, []),
    'emo_grammar_step': (c_i, [ctypes.POINTER(GrammarStep), c_p]),
    'emo_acc_rebase_size': (c_i, []),
    'emo_acc_rebase': (c_i, [ctypes.POINTER(AccRebase), c_p]),
    'emo_accuracy_counts': (c_i, [c_p, c_p, c_p, c_p, c_l, c_l, c_l, c_p, c_p]),
    'emo_sumsq': (c_i, [c_p, c_l, c_p, c_p]),
    'emo_clip_coef': (c_i, [c_p, c_f, c_f, c_p, c_p, c_p]),
    'emo_adam_step': (c_i, [c_p, c_p, c_p, c_p, c_p, c_l, c_f, c_f, c_f, c_f, c_l, c_p, c_p]),
    'emo_cast': (c_i, [c_p, c_i, c_p, c_i, c_l, c_p]),
    'emo_add_bias2': (c_i, [c_p, c_l, c_p, c_p, c_p, c_p, c_i, c_l, c_l, c_p]),
    'emo_transpose_batch': (c_i, [c_p, c_i, c_l, c_p]),
    'emo_stream_wait': (c_i, [c_p, c_p]),
    'emo_comm_bind': (c_i, []),
    'emo_comm_unique_id': (c_i, [c_p]),
    'emo_comm_init': (c_i, [c_p, c_i, c_i]),
    'emo_comm_world': (c_i, []),
    'emo_comm_rank': (c_i, []),
    'emo_comm_allreduce': (c_i, [c_p, c_l, c_i, c_p]),
    'emo_comm_broadcast': (c_i, [c_p, c_l, c_i, c_i, c_p]),
    'emo_comm_destroy': (c_i, []),
}
for _name, (_res, _args) in _SIG.items():
    _fn = getattr(lib, _name)          # AttributeError here = header/library mismatch
    _fn.restype, _fn.argtypes = _res, _args
for _cname, _size, _mirror in (('emo_epilogue_t', lib.emo_epilogue_size, Epilogue), ('emo_decode_step_t', lib.emo_decode_step_size, DecodeStep),
                               ('emo_grammar_step_t', lib.emo_grammar_step_size, GrammarStep), ('emo_attn_t', lib.emo_attn_size, Attn),
                               ('emo_acc_rebase_t', lib.emo_acc_rebase_size, AccRebase)):
    if _size() != ctypes.sizeof(_mirror):                   # a stale libemo_hip.so (or a stale mirror above) would read garbage pointers
        raise ImportError('libemo_hip.so was built with an %s of %d bytes, this binding has %d: rebuild (python -c "import __graft_entry__ as g; g.build()")'
                          % (_cname, _size(), ctypes.sizeof(_mirror)))


class EmoError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise EmoError('libemo_hip error %d: %s' % (rc, lib.emo_last_error().decode()))


def dtype_code(t):
    if t == torch.float32:
        return F32
    if t == torch.bfloat16:
        return BF16
    raise EmoError('unsupported dtype %s (float32 / bfloat16 only)' % t)


def ptr(t):
    """device pointer of a tensor (None -> NULL). Tensors must live on the GPU: no CPU fallback."""
    if t is None:
        return None
    if not t.is_cuda:
        raise EmoError('emo-disentanger_amd ops need GPU tensors (the HIP path has no CPU fallback)')
    return t.data_ptr()


def stream():
    """hipStream_t of torch's current stream on the current device.  (The raw getter: `torch.cuda.current_stream().cuda_stream` builds a Stream
    object through four layers of Python per call — 8.5 us, ~200 calls per training step, a quarter of the host time that BOUNDS the step at the
    reference YAML's batch size 4; tools/b4_host_profile.py, r05.)"""
    return _raw_stream(_cur_device())


# (private torch entry points, present in every torch with a CUDA / ROCm build this package supports; the public form is the fall-back)
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)
if _raw_stream is None or _cur_device is None:
    def stream():                                                  # noqa: F811
        return torch.cuda.current_stream().cuda_stream
